"""`EngineModule`: what every Python class over a librgbd_amd.so engine handle shares -- the checkpoint on the host, the handle
and its device, uploads, and shared-weight clones.  Of entropy coding it knows one thing, the stream-format switch of the codecs (`set_coder`).

    EngineModule                      handle lifecycle
    ├── Spatial_aligner               aligner.py
    ├── SynthesisTransformPlus        aligner.py
    ├── LocalContext, LinearGlobalIntraContext, LinearGlobalInterContext    mlic_context.py
    ├── EntropyParametersMLIC, ChannelContext, LatentResidualPrediction     mlic_slice.py
    └── Codec                         elic_united.py: entropy-table holders, streams, debug / profile hooks
        ├── ELIC_united               elic_united.py (ELIC_united_R2D, SymmetricalTransFormerUnited under it)
        └── SingleCodec               elic.py (ELIC, SymmetricalTransFormer, Cheng2020AnchorwithCheckerboard, MLICPlusPlus under it)

A subclass fills in: `_MODEL` (its name in messages and in synth.synthetic_state_dict), `_synth_args()` (the other keyword
arguments of synth.synthetic_state_dict), `_create_engine()` (one `self._create(...)` line) and, where it sends more than
tensors, `_upload_extras(L)`.  There is no CPU execution path: every call raises if the HIP library or a GPU is missing.
"""
import ctypes
from collections import OrderedDict

import numpy as np
import torch

from . import synth
from ._lib import RgbdError, check, lib


class EngineModule:
    _MODEL = ""
    _CALLS = "the forward pass"  # what _ready() names in its message

    def __init__(self, entries, init_seed=0):
        self._entries = entries  # name -> arch.Entry, in state_dict order
        self._init_seed = init_seed
        self._params = None  # name -> torch CPU tensor (parameters and float buffers)
        self._h = None
        self._device = None
        self._dirty = True
        self._gen = 0        # bumped by every upload of weights / tables to the GPU
        self._parent = None  # set on shared-weight clones (clone_shared)
        self._coder = ("reference", 64)  # set_coder(): the format of the y streams
        self._coder_applied = None       # what the current handle was last told

    # ---- per-class hooks ---------------------------------------------------------------------------------
    def _synth_args(self):
        return {}

    def _create_engine(self):
        raise NotImplementedError

    def _upload_extras(self, L):
        pass

    # ---- torch.nn.Module-like surface ------------------------------------------------------------------
    def _materialize(self):
        if self._params is None:
            self._params = synth.synthetic_state_dict(self._init_seed, model=self._MODEL, **self._synth_args())
        return self._params

    def eval(self):
        return self  # (inference only: `training`, where a class has it, is never True)

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("the MI355X path is inference-only (training is out of scope, DESIGN.md)")
        return self

    def parameters(self):
        p = self._materialize()
        for name, e in self._entries.items():
            if e.is_param:
                yield p[name]

    def count_parameters(self, only_trainable=False):
        return sum(p.numel() for p in self.parameters())

    def state_dict(self):
        p = self._materialize()
        return OrderedDict((name, p[name]) for name in self._entries)

    def load_state_dict(self, state_dict, strict=True):
        """Every parameter must be there (a missing buffer only counts under strict); shapes are checked either way."""
        self._require_owner("load_state_dict")
        missing = [k for k, e in self._entries.items() if k not in state_dict and (e.is_param or strict)]
        unexpected = [k for k in state_dict if k not in self._entries]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for {self._MODEL}: missing {missing[:5]}, unexpected {unexpected[:5]}")
        params = OrderedDict(self._materialize()) if missing else OrderedDict()
        for name, e in self._entries.items():
            if name not in state_dict:
                continue
            v = state_dict[name]
            v = v.detach().cpu() if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))
            if tuple(v.shape) != tuple(e.shape):
                raise RuntimeError(f"size mismatch for {name}: checkpoint {tuple(v.shape)} vs model {tuple(e.shape)}")
            params[name] = v.float().contiguous().clone() if e.is_param else v.clone()
        self._params = params
        self._dirty = True

    def to(self, device):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RgbdError(f"{self._MODEL} (rgbd_amd) runs on the GPU only: use .to('cuda'); there is no CPU path")
        if not torch.cuda.is_available():
            raise RgbdError("no HIP device visible to torch")
        self._device = torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)
        self._upload()
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else f"cuda:{int(device)}")

    # ---- engine ------------------------------------------------------------------------------------
    @staticmethod
    def _create(fn, *args):
        """Call the exported creation function `fn`; a list among its integer arguments goes as (int32 array, length)."""
        h, cargs = ctypes.c_void_p(), []
        for a in args:
            cargs += [(ctypes.c_int32 * len(a))(*a), len(a)] if isinstance(a, list) else [int(a)]
        check(getattr(lib(), fn)(*cargs, ctypes.byref(h)), fn[len("rgbd_"):])
        return h

    def _upload(self):
        L = lib()
        torch.cuda.set_device(self._device)
        if self._h is None:
            self._h = self._create_engine()
        p = self._materialize()
        for name, e in self._entries.items():
            if not e.is_param:
                continue
            a = p[name].detach().float().contiguous().numpy()
            if e.kind == "linear_w" and ".fc." not in name:  # nn.Linear of the Swin blocks -> 1x1 convolution
                a = a.reshape(a.shape[0], a.shape[1], 1, 1)
            shape = (ctypes.c_int64 * a.ndim)(*a.shape)
            check(L.rgbd_elic_set_tensor(self._h, name.encode(), a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), shape,
                                         a.ndim), f"set_tensor({name})")
        self._upload_extras(L)
        check(L.rgbd_elic_finalize(self._h), "finalize")
        self._dirty = False
        self._gen += 1

    def _require_owner(self, what):
        if self._parent is not None:
            raise RgbdError(f"{what}() on a shared-weight clone: call it on the parent engine (clones follow it)")

    def _clone_handle(self, parent):
        h = ctypes.c_void_p()
        check(lib().rgbd_elic_clone_shared(parent._h, ctypes.byref(h)), "clone_shared")
        self._h = h
        self._coder_applied = None  # (a fresh handle starts in the reference format)
        self._gen = parent._gen
        self._params = parent._params

    def _ready(self):
        if self._h is None or self._device is None:
            raise RgbdError(f"call .to('cuda') before {self._CALLS}")
        if self._parent is not None:
            # shared-weight clone: follow the parent.  If the parent has re-uploaded weights or tables since this clone
            # was made (update() / load_state_dict()), take a fresh clone of it -- the old device buffers stay valid
            # until then (they are reference-counted in the library), they are merely stale.
            self._parent._ready()
            if self._parent._gen != self._gen:
                old = self._h
                self._clone_handle(self._parent)
                lib().rgbd_elic_destroy(old)
        elif self._dirty:
            self._upload()
        torch.cuda.set_device(self._device)
        self._apply_coder()

    # ---- stream format of the y strings ------------------------------------------------------------------
    WIDE_TAG = b"RW\x01"  # + bytes([lanes]): the head of every y string of a "wide" engine

    @property
    def coder(self):
        return self.__dict__.get("_coder", ("reference", 64))[0]

    @property
    def coder_lanes(self):
        return self.__dict__.get("_coder", ("reference", 64))[1]

    def set_coder(self, coder="reference", lanes=64):
        """The format of the y strings compress() returns and decompress() expects: "reference" (default; CompressAI's
        streams byte for byte) or "wide" -- `lanes` (1, 2, 4 ... 64) interleaved rANS states coded by one GPU lane each, for
        callers who want a short single call and do not need CompressAI-compatible streams.  A wide y string starts with the
        tag b"RW\x01" + bytes([lanes]) and is 4 + 8 * (lanes - 1) bytes longer; the z strings do not change.  Models whose
        engine has no wide path (STF, STF_united, ELIC_united_R2D, the checkerboard Cheng2020, MLIC++) refuse "wide" here."""
        if coder not in ("reference", "wide"):
            raise ValueError(f"coder must be 'reference' or 'wide', got {coder!r}")
        if coder == "wide" and lanes not in (1, 2, 4, 8, 16, 32, 64):
            raise ValueError(f"lanes must be a power of two in 1 ... 64, got {lanes!r}")
        old = self.__dict__.get("_coder", ("reference", 64))
        self._coder = (coder, int(lanes) if coder == "wide" else 64)
        if self._h is not None:
            try:
                self._apply_coder()
            except RgbdError:
                self._coder = old
                raise
        return self

    def _apply_coder(self):
        want = self.__dict__.get("_coder", ("reference", 64))
        if self._h is None or self.__dict__.get("_coder_applied") == want:
            return
        if want[0] == "reference" and self.__dict__.get("_coder_applied") is None:
            self._coder_applied = want  # a fresh handle is in the reference format already
            return
        check(lib().rgbd_elic_set_coder(self._h, 1 if want[0] == "wide" else 0, want[1]), f"set_coder({want[0]!r})")
        self._coder_applied = want

    def _tag_y(self, strings):
        """y strings as compress() hands them out."""
        if self.coder != "wide":
            return strings
        tag = self.WIDE_TAG + bytes([self.coder_lanes])
        return [tag + s for s in strings]

    def _untag_y(self, strings):
        """y strings as the engine takes them; checked on the host, before anything is launched."""
        if self.coder != "wide":
            return list(strings)
        strings = [bytes(s) for s in strings]
        tag = self.WIDE_TAG + bytes([self.coder_lanes])
        for s in strings:
            if s[:3] != self.WIDE_TAG:
                raise ValueError("coder is 'wide' but a y string has no wide-rANS tag (a reference-format stream?)")
            if s[:4] != tag:
                raise ValueError(f"y string was coded with {s[3]} lanes, this engine is set to {self.coder_lanes}")
        return [s[4:] for s in strings]

    def clone_shared(self):
        """Another engine instance on the same GPU that borrows this one's device weights and tables (own workspace and
        stream).  The clone keeps a reference to its parent so the weights outlive it, and follows its re-uploads."""
        self._ready()
        other = type(self).__new__(type(self))
        other.__dict__.update({k: v for k, v in self.__dict__.items() if k != "_h"})
        other._clone_handle(self)
        other._parent = self
        other._dirty = False
        return other

    @staticmethod
    def _stream_ptr():
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    @staticmethod
    def _ptr(t):
        return ctypes.c_void_p(t.data_ptr())

    def __del__(self):
        try:
            if self._h is not None:
                lib().rgbd_elic_destroy(self._h)
                self._h = None
        except Exception:
            pass
