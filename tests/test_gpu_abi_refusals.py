"""What the engine's entry points refuse, and with which code: family x entry point x handle state -> return code
(csrc/engine_abi.hip).  Every row is a call that is refused on the host before its first kernel launch -- by the readiness
check, the family test or the argument predicate of the entry point, all of which precede use_stream / run_sized -- so no
kernel runs here.  The pointers handed in are real all the same (one zeroed device buffer that holds the largest tensor of any
row, host arrays for the stream arguments): should a predicate regress, the row fails with a wrong return code, not with a
memory fault.  A GPU is needed in any case: creating an engine sets the device's wait policy, tables are uploaded.

The expected codes are those of the library BEFORE the entry points were rewritten over one call frame, recorded by running
this file against that library.  It loads the library itself (ctypes, no argtypes: every argument is an int32 or a pointer)
instead of going through _lib.lib(), so that it runs unchanged against an older librgbd_amd.so named by RGBD_AMD_LIB: the
table holds for both."""
import ctypes
import os

import pytest

from rgbd_amd import _lib

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -22, -1
P, Y, N = "device tensor", "host array of stream pointers", "host array of stream lengths"  # resolved by the `pointers` fixture

CODECS, MODULES = (0, 1, 2, 3, 4, 5), (6, 7, 8, 9)
PAIR, SINGLE = (0, 2, 3), (1, 4, 5)


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib._SO) and "RGBD_AMD_LIB" not in os.environ:
        _lib.build()
    return ctypes.CDLL(_lib._SO)


@pytest.fixture(scope="module")
def pointers():
    import torch

    dev = torch.zeros(1 << 20, dtype=torch.float32, device="cuda:0")  # the largest tensor of a row: up1..up3, 192 x 32 x 32
    data = (ctypes.c_uint8 * 64)()
    streams = (ctypes.c_void_p * 8)(*[ctypes.addressof(data)] * 8)
    lengths = (ctypes.c_int64 * 8)()
    yield {P: ctypes.c_void_p(dev.data_ptr()), Y: streams, N: lengths, "keep": (dev, data)}


def _i32(*v):
    return (ctypes.c_int32 * len(v))(*v)


def create(L, family):
    h = ctypes.c_void_p()
    out = ctypes.byref(h)
    s320, s384 = _i32(16, 16, 32, 64, 192), _i32(24, 24, 48, 96, 192)
    rc = {0: lambda: L.rgbd_elic_create(192, 320, s320, 5, out), 1: lambda: L.rgbd_elic_create_single(192, 320, s320, 5, 3, out),
          2: lambda: L.rgbd_elic_create_stf(192, 384, s384, 5, out), 3: lambda: L.rgbd_elic_create_r2d(192, 320, s320, 5, out),
          4: lambda: L.rgbd_elic_create_stf_single(3, out), 5: lambda: L.rgbd_elic_create_ckbd(128, 3, out),
          6: lambda: L.rgbd_aligner_create(16, 16, out), 7: lambda: L.rgbd_local_context_create(32, out),
          8: lambda: L.rgbd_linear_inter_create(32, 32, 2, out), 9: lambda: L.rgbd_linear_intra_create(32, 2, out)}[family]()
    assert rc == 0 and h.value
    return h


@pytest.fixture(scope="module")
def handles(L):
    """state -> family -> handle.  fresh: created; empty: finalized with no weights and no tables; ready: finalized, with a scale
    table and a (one-row) table in every slot the family reads, so that check_ready passes; clone: a shared-weight clone of empty."""
    hs = {s: {} for s in ("fresh", "empty", "ready", "clone")}
    cdf, sizes, offs, scale = _i32(0, 32768, 65536), _i32(3), _i32(0), (ctypes.c_float * 64)(*[0.11 + i for i in range(64)])
    for f in CODECS + MODULES:
        hs["fresh"][f] = create(L, f)
        hs["empty"][f] = create(L, f)
        assert L.rgbd_elic_finalize(hs["empty"][f]) == 0
        c = ctypes.c_void_p()
        assert L.rgbd_elic_clone_shared(hs["empty"][f], ctypes.byref(c)) == 0
        hs["clone"][f] = c
        if f in CODECS:
            h = hs["ready"][f] = create(L, f)
            assert L.rgbd_elic_finalize(h) == 0
            assert L.rgbd_elic_set_scale_table(h, scale, 64) == 0
            for which in ((0, 1, 2, 3) if f in PAIR else (0, 2)):
                assert L.rgbd_elic_set_tables(h, which, cdf, 3, sizes, offs, 1) == 0
    yield hs
    for per_family in hs.values():
        for h in per_family.values():
            L.rgbd_elic_destroy(h)


# entry point -> its arguments behind the handle, all valid (B = 1; images 64 x 64, latent grids 4 x 4, z grids 1 x 1; module
# maps 8 x 8; the last one is the stream)
VALID = {
    "rgbd_elic_compress": [P, P, 1, 64, 64, 1, None],
    "rgbd_elic_forward": [P, P, 1, 64, 64, P, P, P, P, P, P, None],
    "rgbd_elic_decompress": [Y, N, 1, Y, N, Y, N, Y, N, 1, 1, 1, P, P, None],
    "rgbd_elic_compress_united": [P, P, P, P, 1, 4, 4, 1, None],
    "rgbd_elic_decompress_united": [Y, N, 1, Y, N, P, P, 1, 4, 4, P, P, None],
    "rgbd_elic_compress_single": [P, 1, 64, 64, 1, None],
    "rgbd_elic_forward_single": [P, 1, 64, 64, P, P, P, None],
    "rgbd_elic_decompress_single": [Y, N, 1, Y, N, 1, 1, 1, P, None],
    "rgbd_elic_forward_single_mid": [P, 1, 64, 64, P, P, P, P, P, P, None],
    "rgbd_elic_decompress_single_mid": [Y, N, 1, Y, N, 1, 1, 1, P, P, P, P, None],
    "rgbd_aligner_forward": [P, P, 1, 8, 8, P, None],
    "rgbd_local_context_forward": [P, 1, 8, 8, P, None],
    "rgbd_linear_inter_forward": [P, 1, 8, 8, P, None],
    "rgbd_linear_intra_forward": [P, P, 1, 8, 8, P, None],
}
PAIR_CALLS = ["rgbd_elic_compress", "rgbd_elic_forward", "rgbd_elic_decompress", "rgbd_elic_compress_united", "rgbd_elic_decompress_united"]
SINGLE_CALLS = ["rgbd_elic_compress_single", "rgbd_elic_forward_single", "rgbd_elic_decompress_single"]
MID_CALLS = ["rgbd_elic_forward_single_mid", "rgbd_elic_decompress_single_mid"]
CODEC_CALLS = PAIR_CALLS + SINGLE_CALLS + MID_CALLS
MODULE_CALLS = {"rgbd_aligner_forward": 6, "rgbd_local_context_forward": 7, "rgbd_linear_inter_forward": 8, "rgbd_linear_intra_forward": 9}

# entry point -> {what is wrong: (argument index, value)}: one argument of VALID replaced, which the entry point's predicate
# refuses.  Only pointers the predicate tests are listed (the length arrays of the two-modality decompress calls are not).
BROKEN = {
    "rgbd_elic_compress": {"rgb NULL": (0, None), "depth NULL": (1, None), "B 0": (2, 0), "H % 64": (3, 96), "W % 64": (4, 32)},
    "rgbd_elic_forward": {"rgb NULL": (0, None), "xr NULL": (5, None), "lik_z_depth NULL": (10, None), "H % 64": (3, 96), "W % 64": (4, 100)},
    "rgbd_elic_decompress": {"y_rgb NULL": (0, None), "y_depth NULL": (3, None), "z_rgb NULL": (5, None), "z_depth NULL": (7, None),
                             "xd NULL": (13, None), "n_y 2, B 1": (2, 2), "zh 0": (10, 0)},
    "rgbd_elic_compress_united": {"y_rgb NULL": (0, None), "hyper_depth NULL": (3, None), "odd w": (6, 5), "h 0": (5, 0)},
    "rgbd_elic_decompress_united": {"y_rgb NULL": (0, None), "hyper_rgb NULL": (5, None), "yhat_depth NULL": (11, None),
                                    "odd w": (9, 3), "n_y 2, B 1": (2, 2)},
    "rgbd_elic_compress_single": {"x NULL": (0, None), "H % 64": (2, 32), "W % 64": (3, 65), "B 0": (1, 0)},
    "rgbd_elic_forward_single": {"x NULL": (0, None), "xhat NULL": (4, None), "lik_z NULL": (6, None), "H % 64": (2, 96)},
    "rgbd_elic_decompress_single": {"y NULL": (0, None), "y_len NULL": (1, None), "z NULL": (3, None), "z_len NULL": (4, None),
                                    "x NULL": (8, None), "n_y 2, B 1": (2, 2), "zw 0": (7, 0)},
    "rgbd_elic_forward_single_mid": {"x NULL": (0, None), "up1 NULL": (7, None), "up3 NULL": (9, None), "W % 64": (3, 96)},
    "rgbd_elic_decompress_single_mid": {"y NULL": (0, None), "up2 NULL": (10, None), "n_y 2, B 1": (2, 2)},
    "rgbd_aligner_forward": {"x NULL": (0, None), "guided NULL": (1, None), "out NULL": (5, None), "H % 8": (3, 12), "W % 8": (4, 4), "B 0": (2, 0)},
    "rgbd_local_context_forward": {"x NULL": (0, None), "out NULL": (4, None), "H 0": (2, 0)},
    "rgbd_linear_inter_forward": {"x1 NULL": (0, None), "out NULL": (4, None), "W 0": (3, 0)},
    "rgbd_linear_intra_forward": {"x1 NULL": (0, None), "x2 NULL": (1, None), "out NULL": (5, None), "odd W": (4, 7)},
}


def rows():
    """(id, state, family or None, entry point, arguments, expected code)"""
    out = []
    for call in CODEC_CALLS:  # no handle: nothing is ready; the module calls test the family first
        out.append((f"null-{call}", None, None, call, VALID[call], ESTATE))
    for call in MODULE_CALLS:
        out.append((f"null-{call}", None, None, call, VALID[call], EINVAL))
    for state in ("fresh", "empty"):  # not ready: a codec says so, a module handle has no codec calls at all
        for f in CODECS + MODULES:
            for call in CODEC_CALLS:
                out.append((f"{state}-f{f}-{call}", state, f, call, VALID[call], ESTATE if f in CODECS else EINVAL))
    for state in ("fresh", "empty", "ready"):  # a module call on a handle of another family, whatever its state
        for f in CODECS + MODULES:
            for call, own in MODULE_CALLS.items():
                if f != own and (state != "ready" or f in CODECS):
                    out.append((f"{state}-f{f}-{call}", state, f, call, VALID[call], EINVAL))
    for call, own in MODULE_CALLS.items():
        out.append((f"fresh-f{own}-{call}", "fresh", own, call, VALID[call], ESTATE))  # its own family, not finalized
        for what, (i, v) in BROKEN[call].items():  # finalized: the argument predicate
            out.append((f"empty-f{own}-{call}-{what}", "empty", own, call, VALID[call][:i] + [v] + VALID[call][i + 1:], EINVAL))
    for f in CODECS:  # ready codecs: the family test and the argument predicate of each entry point
        for call in SINGLE_CALLS + MID_CALLS:
            if f in PAIR or (call in MID_CALLS and f != 1):
                out.append((f"ready-f{f}-{call}", "ready", f, call, VALID[call], EINVAL))
        mine = PAIR_CALLS if f in PAIR else SINGLE_CALLS + (MID_CALLS if f == 1 else [])
        for call in mine:
            for what, (i, v) in BROKEN[call].items():
                out.append((f"ready-f{f}-{call}-{what}", "ready", f, call, VALID[call][:i] + [v] + VALID[call][i + 1:], EINVAL))
    return out


ROWS = rows()


@pytest.mark.parametrize("state, family, call, args, code", [r[1:] for r in ROWS], ids=[r[0] for r in ROWS])
def test_refused(L, handles, pointers, state, family, call, args, code):
    h = handles[state][family] if state else None
    assert getattr(L, call)(h, *[pointers[a] if isinstance(a, str) else a for a in args]) == code


@pytest.mark.parametrize("family", CODECS + MODULES)
def test_finalize_refuses_a_clone(L, handles, family):
    assert L.rgbd_elic_finalize(handles["clone"][family]) == ESTATE


def test_table_shape():
    assert len({r[0] for r in ROWS}) == len(ROWS) > 400
    for r in ROWS:  # no row with every argument valid on a handle that could run it
        state, f, call, args = r[1:5]
        runnable = (state == "ready" and call in CODEC_CALLS) or (state == "empty" and MODULE_CALLS.get(call) == f)
        if runnable and args == VALID[call]:
            assert (call in SINGLE_CALLS + MID_CALLS) and (f in PAIR or (call in MID_CALLS and f != 1)), r[0]
