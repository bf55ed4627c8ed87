"""What the Python model classes show of themselves without a GPU: constructor attributes, state_dict keys, parameter
count, public names, and the library calls an upload makes.  tools/record_model_surface.py writes these fields, on the commit
to compare AGAINST, into tests/golden/model_surface_record.json; tests/test_model_surface.py holds the present classes to
that record.

The upload log: `lib` of every model module (not of entropy_models, whose table builders need the real library) is replaced by
a stub that answers 0 to every call (1 to rgbd_elic_get_refnum) and keeps the function name and every argument that is a
Python int, bytes or a ctypes array of integers ("*" stands for a pointer).  It holds integers and names only."""
import ctypes
import hashlib
import json
import sys
from collections import Counter

import torch

CLASSES = ["ELIC_united_R2D", "ELIC_united", "ELIC", "STF_united", "STF", "ckbd", "Spatial_aligner"]
_INT_TYPES = (ctypes.c_int8, ctypes.c_int16, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint8, ctypes.c_uint16, ctypes.c_uint32,
              ctypes.c_uint64)


def make(name, **kw):
    import rgbd_amd

    return rgbd_amd.Spatial_aligner(**kw) if name == "Spatial_aligner" else rgbd_amd.modelZoo[name](**kw)


def _arg(a):
    if isinstance(a, bytes):
        return a.decode()
    if isinstance(a, int):
        return int(a)
    if isinstance(a, ctypes.Array) and a._type_ in _INT_TYPES:
        return list(a)
    return "*"


class RecordingLib:
    def __init__(self):
        self.log = []

    def __getattr__(self, fn):
        def call(*args):
            self.log.append([fn] + [_arg(a) for a in args])
            return 1 if fn == "rgbd_elic_get_refnum" else 0

        return call


def upload_log(net):
    """The calls net._upload() makes, with the tables of update(force=True) where the class has one."""
    rec = RecordingLib()
    mods = {sys.modules[c.__module__] for c in type(net).__mro__ if c is not object}  # the modules the class is written in
    mods = [m for m in mods if hasattr(m, "lib")]
    saved = [(m, m.lib) for m in mods]
    set_device = torch.cuda.set_device
    try:
        for m in mods:
            m.lib = lambda: rec
        torch.cuda.set_device = lambda d: None
        if hasattr(net, "update"):
            net.update(force=True)
        net._device = torch.device("cuda", 0)
        net._upload()
    finally:
        torch.cuda.set_device = set_device
        for m, f in saved:
            m.lib = f
        net._h = None  # (no engine was created: nothing to destroy)
    return rec.log


def _plain(v):
    return isinstance(v, (bool, int, float, str)) or (isinstance(v, (list, tuple)) and all(isinstance(x, (bool, int, float, str)) for x in v))


def _sha(obj):
    return hashlib.sha256(json.dumps(obj, separators=(",", ":")).encode()).hexdigest()


def surface(name):
    net = make(name)
    attrs = {k: (list(v) if isinstance(v, tuple) else v) for k, v in vars(net).items() if not k.startswith("_") and _plain(v)}
    sd = net.state_dict()
    out = {"attributes": attrs,
           # the ordered (key, shape, dtype) list is some 4,700 entries over the seven classes: its length and hash are kept
           "state_dict_keys": len(sd),
           "state_dict_sha256": _sha([[k, list(v.shape), str(v.dtype)] for k, v in sd.items()]),
           # (Spatial_aligner had no count_parameters() when the record was made: the sum over its parameter entries then)
           "count_parameters": int(net.count_parameters()) if hasattr(net, "count_parameters") else
           int(sum(sd[k].numel() for k, e in net._entries.items() if e.is_param)),
           "public_names": sorted(n for n in dir(net) if not n.startswith("_"))}
    log = upload_log(net)
    out["upload_sha256"] = _sha(log)
    out["upload_calls"] = dict(sorted(Counter(c[0] for c in log).items()))
    return out
