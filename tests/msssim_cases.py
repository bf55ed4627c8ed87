"""Cases shared by tests/test_msssim_cases.py (CPU: can the checks fail?) and tests/test_gpu_msssim.py (GPU: the three kernels
of csrc/metrics.hip ALONE, through the C ABI's rgbd_msssim_stats, whose out[P][5][2] -- the mean SSIM and the mean
contrast-structure (CS) of every plane at every scale -- is what is judged, not the scalar the wrapper folds it into).

For every case: deterministic planes x, y [P][H][W] fp32 of several input families, the fp64 statement of the definition
(`stats64`: oracle/msssim_ref.py's stats(), no relu, no weights), an fp32 CPU restatement of what the kernels do (`emulate`,
with deliberately wrong variants) and ONE acceptance function (`accept`) that the restatement, its mutants and the GPU
output all go through.

The restatement follows the kernels step by step on torch CPU tensors: clamp at load; the five maps x, y, x^2, y^2, xy through
the horizontal and then the vertical 11-tap pass, each tap an fmaf (the exact product and the sum in fp64, then one rounding to
fp32); the two ratios in plain fp32 (the library is built with -ffp-contract=off); the sum of a 16 x 64 tile as the kernel's 256
threads add it (four rows each, then the fixed tree), the tiles in workgroup order, times fp32(1 / ((h - 10)(w - 10))); the
2 x 2 pool with pad (h % 2, w % 2) on both sides, taps added in (dy, dx) order, times 0.25.

Bound of every (case, scale, statistic), fixed when the case is built and before any kernel runs:
    |got - ref64| <= 4 * max(E32, 8 * 2^-24 * max(1, |ref64|))
E32: the worst distance over the case's planes between emulate(case) and stats64 at that scale and statistic -- what fp32
arithmetic of this shape costs on these very inputs (fp32 taps that do not sum to one, E[x^2] - mu^2 against c2 = 9e-4).  The
factor 4 pays for a summation order or a rounding the restatement does not share; the floor for cases where the restatement
happens to be exact.  `stats` receives the worst err / max(E32, floor) of the case ("ratio": at most 1 for the restatement, at
most 4 for an accepted output).

Input families (one letter per plane in CASES):
  a  smooth pattern against itself plus Gaussian noise 0.05          b  two independent uniform planes
  c  a pattern against 1 - pattern: every CS is negative              d  dark planes in [0, 0.004]: the luminance factor and c1
  e  flat bright planes, 0.97 plus noise 0.002: the cancellation      g  x == y: every statistic is 1
  f  family a stretched to [-0.5, 1.5]   n  family c stretched likewise   u  uniform in [-0.5, 1.5]   (clamp01 = 1 and = 0)
  family h is a / c scaled by the case's `scale`, run with data_range = scale (255 and 0.5)

Measured.  E32 is the largest over the ten (scale, statistic) pairs, on the CPU; "kernel" is the kernel's worst ratio on an
MI355X (gfx950), allowed 4:
    case         E32 at scale 0 (ssim, cs)   largest E32 (always scale 4)   kernel
    min_odd      3.1e-6, 3.2e-6              2.05e-5 (the flat bright plane)  1.000
    exact_tiles  9.5e-7, 8.7e-7              1.31e-5                          1.000
    one_over     1.1e-6, 1.2e-6              2.18e-5                          1.000
    wide         1.1e-6, 1.3e-6              9.94e-6                          1.000
    tall         1.1e-6, 1.1e-6              1.43e-5                          1.000
    planes65     1.8e-6, 1.7e-6              9.56e-5                          1.000
    clamp1       3.5e-7, 3.7e-7              8.37e-6                          1.000
    clamp0       1.7e-7, 2.2e-7              8.75e-6                          1.000
    range255     1.2e-6, 9.5e-7              3.15e-5                          1.000
    range_half   1.1e-6, 1.0e-6              1.41e-5                          1.000
The ratio is 1.000 everywhere because the kernel returned the restatement's very bits: all 920 statistics of the ten cases were
bit-identical to emulate() (the test prints that count; it asserts the bound).  E32 itself is mostly the fp32 taps, which sum to
1 - 3e-8 where the fp64 window sums to 1: E[x^2] - mu^2 then carries -delta mu^2, seen against c2 = 9e-4, and the coarse scales
inherit four pools of it.
"""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import msssim_ref

f32 = np.float32
EPS24 = 2.0 ** -24
KT, TH, TW = 11, 16, 64  # taps, output tile of one workgroup (csrc/metrics.hip)
CAP = 1e-3               # no E32 may reach this (tests/test_msssim_cases.py): a broken restatement cannot open the bound

# (id, P, H, W, families of the planes (cycled, every plane its own seed), data_range = scale of the planes, clamp01)
# (every case has at least three planes of different content, a plane with CS < 0 and one with CS > 0.9 at scale 0)
CASES = [
    ("min_odd", 3, 161, 161, "ecd", 1.0, 1),      # smallest legal: 161 -> 81 -> 41 -> 21 -> 11, every pool pads, scale 4's map is 1 x 1
    ("exact_tiles", 3, 170, 202, "gca", 1.0, 1),  # scale-0 map 160 x 192: exactly 10 x 3 tiles
    ("one_over", 3, 171, 203, "acb", 1.0, 1),     # scale-0 map 161 x 193: a last tile of one row, one of one column; 203 -> 102 -> 51 -> 26 -> 13
    ("wide", 3, 163, 400, "acd", 1.0, 1),         # many tiles across, one partial
    ("tall", 3, 400, 162, "bcg", 1.0, 1),         # the transpose, even -> odd chain
    ("planes65", 65, 161, 170, "abcdegf", 1.0, 1),  # second block of the finish kernel, plane stride of the partials
    ("clamp1", 3, 161, 170, "fnu", 1.0, 1),       # family f, clamped by the kernel
    ("clamp0", 3, 161, 170, "fnu", 1.0, 0),       # family f, as it is
    ("range255", 3, 161, 170, "aca", 255.0, 0),   # family h
    ("range_half", 3, 161, 170, "aca", 0.5, 0),
]
IDS = [c[0] for c in CASES]
SMALL = [i for i in IDS if i != "planes65"]

# the deliberately wrong restatements accept() must reject on at least one case
MUTANTS = ["drop_pixel", "edge_row", "edge_col", "count", "pool_divisor", "pool_pad", "c_swap", "range", "no_clamp", "always_clamp",
           "clamp_pool_after", "clamp_pool_skip", "plane", "slot", "scale"]


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) % (2 ** 31))


def case_id(c):
    return c["id"]


def sides(n):
    """the chain of one side over the five scales (F.avg_pool2d(kernel 2, padding n % 2))"""
    out = [n]
    for _ in range(4):
        n = (n + 2 * (n % 2) - 2) // 2 + 1
        out.append(n)
    return out


# ================================================================================================ inputs
def _pattern(rng, H, W):
    """smooth and of high contrast, in [0.02, 0.98]: a diagonal sinusoid of period 8 ... 14 pixels along each axis (fine enough to
    give the 11-tap window a local variance far above c2) and two of periods 12 ... 40"""
    r, c = np.arange(H, dtype=np.float64)[:, None], np.arange(W, dtype=np.float64)[None, :]
    p = np.concatenate([rng.uniform(8, 14, 2), rng.uniform(12, 40, 3)])
    ph = rng.uniform(0, 2 * np.pi, 3)
    return (0.5 + 0.25 * np.sin(2 * np.pi * (r / p[0] + c / p[1]) + ph[0]) + 0.15 * np.sin(2 * np.pi * (r / p[2] - c / p[3]) + ph[1])
            + 0.08 * np.sin(2 * np.pi * c / p[4] + ph[2]))


def family_planes(fam, key, H, W):
    """one plane pair (x, y) [H][W] fp32 of family `fam`, deterministic from `key`"""
    rng = _rng("msssim", fam, key, H, W)
    pat = _pattern(rng, H, W)
    if fam == "a":
        x, y = pat, pat + 0.05 * rng.standard_normal((H, W))
    elif fam == "b":
        x, y = rng.uniform(0, 1, (H, W)), rng.uniform(0, 1, (H, W))
    elif fam == "c":
        x, y = pat, 1.0 - pat
    elif fam == "d":
        x = 0.004 * (0.6 + 0.4 * (0.9 * pat + 0.1 * rng.uniform(0, 1, (H, W))))  # (local means apart: the luminance factor leaves 1)
        y = 0.004 * 0.2 * (0.9 * _pattern(rng, H, W) + 0.1 * rng.uniform(0, 1, (H, W)))
    elif fam == "e":
        x, y = 0.97 + 0.002 * rng.standard_normal((H, W)), 0.97 + 0.002 * rng.standard_normal((H, W))
    elif fam == "g":
        x = np.clip(pat + 0.1 * rng.standard_normal((H, W)), 0, 1)
        y = x
    elif fam == "f":
        x = 2 * pat - 0.5
        y = x + 0.1 * rng.standard_normal((H, W))
    elif fam == "n":
        x = 2 * pat - 0.5
        y = 1.0 - x
    elif fam == "u":
        x, y = rng.uniform(-0.5, 1.5, (H, W)), rng.uniform(-0.5, 1.5, (H, W))
    else:
        raise KeyError(fam)
    return x.astype(f32), y.astype(f32)


def taps32():
    """the eleven fp32 taps metrics.ms_ssim_gpu hands the library"""
    from rgbd_amd.metrics import _gauss

    return _gauss().numpy()


# ================================================================================================ the definition, fp64
def stats64(x, y, data_range, clamp01):
    """[P][5][2] fp64 = (mean SSIM, mean CS) of every plane and scale from the definition: no relu, no weights"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if clamp01:
        x, y = np.clip(x, 0.0, 1.0), np.clip(y, 0.0, 1.0)
    return msssim_ref.stats(x, y, data_range)


def luminance64(x, y, data_range=1.0):
    """[P] fp64: the mean of the luminance factor (2 mu1 mu2 + c1) / (mu1^2 + mu2^2 + c1) at scale 0"""
    g = msssim_ref._window()
    c1 = (0.01 * data_range) ** 2
    mu1, mu2 = msssim_ref._blur(np.asarray(x, np.float64), g), msssim_ref._blur(np.asarray(y, np.float64), g)
    return ((2 * mu1 * mu2 + c1) / (mu1 * mu1 + mu2 * mu2 + c1)).mean(axis=(-2, -1))


# ================================================================================================ the kernels, restated
def _fmaf(g, a, s):
    """fmaf(g, a, s) on fp32 tensors: the product of two fp32 numbers is exact in fp64"""
    return (a.double() * g + s.double()).float()


def _filter(x, taps, dim):
    n = x.shape[dim] - (KT - 1)
    s = torch.zeros_like(x.narrow(dim, 0, n))
    for k in range(KT):
        s = _fmaf(float(taps[k]), x.narrow(dim, k, n), s)
    return s


def _tile_sums(m, inv):
    """[P][oh][ow] -> [P]: every 16 x 64 tile as its workgroup adds it (thread tid: rows tid / 64 + 4 j of column tid % 64, then
    the tree over the 256 threads), the tiles in workgroup order, times inv"""
    P, oh, ow = m.shape
    ty, tx = -(-oh // TH), -(-ow // TW)
    z = F.pad(m, (0, tx * TW - ow, 0, ty * TH - oh)).view(P, ty, 4, 4, tx, TW)  # row = 16 tile + 4 j + q
    acc = z[:, :, 0]
    for j in range(1, 4):
        acc = acc + z[:, :, j]
    v = acc.permute(0, 1, 3, 2, 4).reshape(P, ty * tx, 256)  # [.., q, c] -> tid = 64 q + c
    o = 128
    while o:
        v = v[..., :o] + v[..., o:2 * o]
        o >>= 1
    s = torch.zeros(P, dtype=torch.float32)
    for b in range(ty * tx):
        s = s + v[:, b, 0]
    return s * inv


def _pool(x, mutant):
    h, w = x.shape[-2:]
    ph, pw = h % 2, w % 2
    oh, ow = (h + 2 * ph - 2) // 2 + 1, (w + 2 * pw - 2) // 2 + 1
    pad = (0, pw, 0, ph) if mutant == "pool_pad" else (pw, pw, ph, ph)

    def add4(t):
        z = F.pad(t, pad)[..., :2 * oh, :2 * ow]
        return ((z[..., 0::2, 0::2] + z[..., 0::2, 1::2]) + z[..., 1::2, 0::2]) + z[..., 1::2, 1::2]

    if mutant == "pool_divisor":
        return add4(x) / add4(torch.ones_like(x))
    return add4(x) * 0.25


def emulate(case, mutant=None):
    """[P][5][2] fp32: the kernels' arithmetic on the case's planes (module docstring); `mutant`: one of MUTANTS"""
    assert mutant is None or mutant in MUTANTS, mutant
    x, y = torch.tensor(case["x"]), torch.tensor(case["y"])
    P = x.shape[0]
    dr = f32(1.0) if mutant == "range" else f32(case["data_range"])
    c1, c2 = float((f32(0.01) * dr) * (f32(0.01) * dr)), float((f32(0.03) * dr) * (f32(0.03) * dr))
    if mutant == "c_swap":
        c1, c2 = c2, c1
    taps = case["taps"]
    cl = (bool(case["clamp01"]) and mutant != "no_clamp") or mutant == "always_clamp"
    out = torch.zeros(P, 5, 2, dtype=torch.float32)
    for sc in range(5):
        h, w = x.shape[-2:]
        a, b = (x.clamp(0, 1), y.clamp(0, 1)) if cl else (x, y)
        m = [_filter(_filter(t, taps, 2), taps, 1) for t in (a, b, a * a, b * b, a * b)]  # horizontal, then vertical
        mu1, mu2 = m[0], m[1]
        s1, s2, s12 = m[2] - mu1 * mu1, m[3] - mu2 * mu2, m[4] - mu1 * mu2
        cs = (2 * s12 + c2) / (s1 + s2 + c2)
        ss = ((2 * mu1 * mu2 + c1) / (mu1 * mu1 + mu2 * mu2 + c1)) * cs
        oh, ow = h - (KT - 1), w - (KT - 1)
        if mutant == "drop_pixel" and sc == 0:  # the last pixel of workgroup 0's tile
            ss, cs = ss.clone(), cs.clone()
            ss[:, TH - 1, TW - 1] = cs[:, TH - 1, TW - 1] = 0
        if mutant == "edge_row":  # the last tile row stops one output row early
            ss, cs = ss.clone(), cs.clone()
            ss[:, oh - 1, :] = cs[:, oh - 1, :] = 0
        if mutant == "edge_col":
            ss, cs = ss.clone(), cs.clone()
            ss[:, :, ow - 1] = cs[:, :, ow - 1] = 0
        inv = float(f32(1.0) / (f32(h) * f32(w))) if mutant == "count" else float(f32(1.0) / (f32(oh) * f32(ow)))
        out[:, sc, 0], out[:, sc, 1] = _tile_sums(ss, inv), _tile_sums(cs, inv)
        if sc < 4:
            if mutant == "clamp_pool_after" and cl:  # the pool clamps what it wrote, not what it read
                x, y = _pool(x, mutant).clamp(0, 1), _pool(y, mutant).clamp(0, 1)
            elif mutant == "clamp_pool_skip":  # the pool does not clamp: the later scales see the raw values
                x, y = _pool(x, mutant), _pool(y, mutant)
            else:
                x, y = _pool(a, mutant), _pool(b, mutant)
            cl = False  # (already clamped)
    if mutant == "plane":
        out = out[[1, 0] + list(range(2, P))]
    elif mutant == "slot":
        out = out.flip(2)
    elif mutant == "scale":
        out = torch.cat([torch.zeros(P, 1, 2), out[:, :4]], dim=1)
    return out.numpy()


# ================================================================================================ cases
@functools.lru_cache(maxsize=None)
def build(cid):
    _, P, H, W, fams, scale, clamp01 = next(c for c in CASES if c[0] == cid)
    xs, ys, fam = [], [], []
    seed = "clamp" if cid in ("clamp0", "clamp1") else cid  # (the same planes with and without the clamp)
    for p in range(P):
        fam.append(fams[p % len(fams)])
        a, b = family_planes(fam[-1], (seed, p), H, W)
        xs.append(a * f32(scale))
        ys.append(b * f32(scale))
    c = {"id": cid, "P": P, "H": H, "W": W, "fam": fam, "data_range": float(scale), "clamp01": int(clamp01),
         "x": np.ascontiguousarray(np.stack(xs)), "y": np.ascontiguousarray(np.stack(ys)), "taps": taps32()}
    c["ref"] = stats64(c["x"], c["y"], c["data_range"], c["clamp01"])
    c["emu"] = emulate(c)
    c["E32"] = np.abs(c["emu"].astype(np.float64) - c["ref"]).max(axis=0)  # [5][2]: the worst over the planes
    c["floor"] = 8 * EPS24 * np.maximum(1.0, np.abs(c["ref"]))           # [P][5][2]
    c["unit"] = np.maximum(c["E32"][None], c["floor"])
    for k in ("x", "y", "taps", "ref", "emu", "E32", "floor", "unit"):
        c[k].setflags(write=False)
    return c


def accept(case, got, stats=None):
    """-> list of failures (empty: accepted).  got: [P][5][2] (any float type).  Nothing here comes from `got` but the error."""
    got = np.asarray(got)
    if got.shape != case["ref"].shape:
        return [f"shape {got.shape}, want {case['ref'].shape}"]
    err = np.abs(got.astype(np.float64) - case["ref"])
    ratio = err / case["unit"]
    ratio = np.where(np.isfinite(ratio), ratio, np.inf)
    if stats is not None:
        stats.update({"ratio": float(ratio.max()), "E32": float(case["E32"].max()),
                      "per_scale": [[float(ratio[:, s, k].max()) for k in range(2)] for s in range(5)]})
    fails = []
    for s in range(5):
        for k, name in enumerate(("ssim", "cs")):
            bad = np.flatnonzero(~(ratio[:, s, k] <= 4.0))
            if bad.size:
                p = int(bad[np.argmax(ratio[bad, s, k])])
                fails.append(f"{case['id']} scale {s} {name}: {bad.size} of {case['P']} planes outside 4 x {case['unit'][p, s, k]:.3g}; "
                             f"worst plane {p} ({case['fam'][p]}): got {got[p, s, k]!r}, fp64 {case['ref'][p, s, k]!r}")
    return fails
