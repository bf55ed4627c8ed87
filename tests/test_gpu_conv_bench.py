"""rgbd_conv_bench alone (csrc/hooks_abi.hip): the entry point every number in csrc/tile_table*.h and csrc/splitk_table.h was
timed through.  Each case is one call with two timed iterations on a tiny shape, under the conv shape log: the call must
succeed, report a finite positive time, and have launched exactly the shape the arguments and the debug switches describe --
one warm-up launch plus the timed ones.

The expected keys (N,H,W,cin_pad,cout_pad,ntaps,stride,nphase,splitk) follow from the arguments and from how launch_conv_main
(csrc/conv_mfma.hip) writes the log: the stride field is the output step of a transposed conv, the nphase field carries + 100
for the blocked-accumulation kernels, the splitk field is the split factor after the launcher's clamp to cin_pad / 16."""
import ctypes
import math

import pytest

from gpu_utils import require_gpu

pytestmark = pytest.mark.gpu

ITERS = 2

# (n, cin, h, w, cout, k, stride, pad, transposed, with_residual)
CONV3 = (1, 32, 9, 9, 48, 3, 1, 1, 0, 0)
KEY3 = "1,9,9,32,48,9,1,1,1"

# id: (arguments, debug switches {setter: (value, value to restore)}, expected key, launches)
CASES = {
    "3x3": (CONV3, {}, KEY3, ITERS + 1),
    "3x3-splitk2": (CONV3, {"rgbd_debug_force_splitk": (2, 0)}, "1,9,9,32,48,9,1,1,2", ITERS + 1),
    "3x3-blocked": (CONV3, {"rgbd_debug_force_blocked": (1, 0)}, "1,9,9,32,48,9,1,101,1", ITERS + 1),
    # 1x1 layers take a block per 96 channels: 208 = 96 + 96 + 16
    "1x1-blocked": ((1, 208, 8, 8, 32, 1, 1, 0, 0, 0), {"rgbd_debug_force_blocked": (1, 0)}, "1,8,8,208,32,1,1,101,1", ITERS + 1),
    "5x5-transposed": ((1, 32, 5, 5, 16, 5, 2, 2, 1, 0), {}, "1,5,5,32,16,25,2,4,1", ITERS + 1),
    "3x3-residual": (CONV3[:9] + (1,), {}, KEY3, ITERS + 1),
    # loaded mode: the warm-up launch, then every timed iteration once per stream
    "3x3-streams2": (CONV3, {"rgbd_debug_bench_streams": (2, 1)}, KEY3, 1 + ITERS * 2),
}


def _log_read(L):
    need = L.rgbd_debug_conv_log_read(None, 0)
    buf = ctypes.create_string_buffer(int(need))
    L.rgbd_debug_conv_log_read(buf, need)
    rows = [line.rsplit(",", 1) for line in buf.value.decode().splitlines()[1:] if line]
    return {key: int(count) for key, count in rows}


@pytest.mark.parametrize("case", list(CASES), ids=str)
def test_conv_bench_launches_the_shape_it_is_asked_for(case):
    require_gpu()
    from rgbd_amd._lib import check, lib

    L = lib()
    args, switches, key, launches = CASES[case]
    ms = ctypes.c_float(float("nan"))
    try:
        for setter, (value, _) in switches.items():
            check(getattr(L, setter)(value), setter)
        check(L.rgbd_debug_conv_log(1), "conv_log")
        rc = L.rgbd_conv_bench(*args, ITERS, ctypes.byref(ms))
        log = _log_read(L)
    finally:
        L.rgbd_debug_conv_log(0)
        for setter, (_, restore) in switches.items():
            getattr(L, setter)(restore)
    assert rc == 0
    assert math.isfinite(ms.value) and ms.value > 0
    assert log == {key: launches}
