"""Cases shared by tests/test_gdn_cases.py (CPU: can the checks fail?) and tests/test_gpu_gdn.py (GPU: the fused GDN / IGDN
launch of csrc/gdn.hip ALONE, in the engine's layout, through the C ABI's rgbd_gdn_pack / rgbd_gdn_nhwc).

    y[p][i] = x[p][i] * f(beta'[i] + sum_j gamma'[i][j] * x[p][j]^2)  (+ res[p][i]),   f = 1 / sqrt (GDN) or sqrt (IGDN)

For every case: raw parameters and inputs from the recipe of tests/test_gpu_gdn.py (dense gamma with a share below the
parametrizer's bound, a different beta per channel, |x| from 1e-3 to 1e2 with exact zeros and one all-zero pixel), laid out
as the engine's NHWC buffers with one channel stride per tensor:

    x   [npix][xcs]: channels [0, c) the values, [c, cs) zero (the engine's pad), [cs, xcs) NaN (never to be read)
    res [npix][rcs]: likewise
    y   [npix][ycs]: SENTINEL everywhere, followed by a guard band of SENTINEL

(cs = c rounded up to 16).  All three buffers are TAIL pixels longer than npix (x: zeros, res: zeros, y: the guard band), so
that a launch that ran a whole 64-pixel tile past npix would still stay inside them.

Reference: the formula in float64 from the fp32 parametrized beta' / gamma' (NonNegativeParametrizer.forward in torch fp32).

Acceptance (`accept`, the one function the CPU restatement, its wrong variants and the GPU outputs all go through):
  * per element of channels [0, c):  |y - ref| <= ((c / 2 + 4) * |x f(norm)| + |ref|) * 2^-24.  This is the bound of
    tests/test_gpu_gdn.py, derived there from the arithmetic: every term of the norm is non-negative, so the bound does not
    depend on the order of the sum and needs no measurement;
  * exactly: x == 0 gives the residual, or +0 without one;
  * exactly: the pad channels [c, cs) of y are +0 (the residual's pad is +0);
  * channels [cs, ycs) of y and the guard band keep SENTINEL bit for bit;
  * no NaN anywhere in the buffer.

`emulate` restates the launch in numpy fp32 on the laid-out buffers, tile by tile as the kernel walks them (P pixels per
workgroup, WS waves per 16 pixels each with its own range of 16-channel output tiles, IT output tiles per pass): beta first,
then the products one by one in the kernel's order, then sqrt / divide / multiply / add, each rounded.  MUTANTS are the same
restatement with one deliberate mistake each.
"""
import functools

import numpy as np
import torch

f32 = np.float32
SENTINEL = f32(12345.0)
TAIL = 64            # pixels behind npix in every buffer: the largest pixel tile
EPS24 = 2.0 ** -24

# the launcher's constants (csrc/gdn.hip), restated
IT = 12              # kGdnIT: 16-channel output tiles a wave accumulates per pass
MAX_C = 512          # kGdnMaxC
TILES = (16, 32, 64)


def round_up(v, m):
    return (v + m - 1) // m * m


def tile_for(npix, cs):
    """gdn_tile_for: the largest tile that still gives 512 workgroups, at most 32 pixels above 256 channels; else 16"""
    p = 32 if cs > 256 else 64
    while p > 16:
        if npix // p >= 512:
            return p
        p >>= 1
    return 16


def waves_per_16(tile):
    return 4 if tile == 16 else 1


# ================================================================================================ cases
def _mk(group, c, npix, d=(0, 0, 0)):
    cs = round_up(c, 16)
    cid = f"{group}-c{c}-n{npix}" + ("" if d == (0, 0, 0) else "-s%d.%d.%d" % d)
    return dict(id=cid, group=group, c=c, cs=cs, npix=npix, xcs=cs + d[0], ycs=cs + d[1], rcs=cs + d[2])


STRIDES = [(0, 0, 0), (4, 0, 0), (0, 12, 0), (0, 0, 20), (16, 4, 36)]  # what each stride is above cs: x, y, res
CASES = ([_mk("chan", c, 37) for c in (16, 80, 112, 200, 272, 320, 384, 500)] +
         [_mk("pix", 208, n) for n in (1, 15, 16, 17, 31, 33, 63, 64, 65)] +
         [_mk("stride", 200, 37, d) for d in STRIDES[1:]] + [_mk("stride", 16, 37, STRIDES[4]), _mk("stride", 500, 37, STRIDES[4])] +
         [_mk("auto", 16, 32768 + 5), _mk("auto", 16, 16384 + 3), _mk("auto", 272, 32768 + 5)])
AUTO_TILE = {"auto-c16-n32773": 64, "auto-c16-n16387": 32, "auto-c272-n32773": 32}  # what gdn_tile_for must choose there
BY_ID = {c["id"]: c for c in CASES}
SMALL = [c["id"] for c in CASES if c["group"] != "auto"]
COMBOS = [(0, 0), (0, 1), (1, 0), (1, 1)]  # (inverse, with_res)


def dense_id(case):
    """the case with the same data and all three strides equal to cs"""
    return f"chan-c{case['c']}-n{case['npix']}"


# ================================================================================================ inputs
def params(c, seed):
    """Raw beta [c] / gamma [c, c] as a state_dict holds them (before NonNegativeParametrizer.forward)."""
    g = torch.Generator().manual_seed(1000 + seed)
    beta = torch.sqrt(0.2 + 2.0 * torch.rand(c, generator=g))  # beta' in 0.2 ... 2.2, a different one per channel
    gamma = 0.08 * torch.rand(c, c, generator=g) - 0.015       # dense; about a fifth of it below the bound 2^-18
    gamma += torch.sqrt(torch.tensor(0.1)) * torch.eye(c)
    return beta.float().contiguous(), gamma.float().contiguous()


def parametrized(raw, minimum):
    """NonNegativeParametrizer.forward (ops/parametrizers.py:21-45) as torch computes it in fp32."""
    pedestal = torch.tensor([(2.0 ** -18) ** 2], dtype=torch.float32)
    bound = torch.tensor([(minimum + (2.0 ** -18) ** 2) ** 0.5], dtype=torch.float32)
    return torch.max(raw, bound) ** 2 - pedestal


def inputs(c, npix, seed):
    """x, res [npix, c] fp32: magnitudes 1e-3 ... 1e2, a tenth exact zeros, pixel npix / 2 all zero (where there are two)."""
    g = torch.Generator().manual_seed(seed)
    shape = (npix, c)
    mag = 10.0 ** (5.0 * torch.rand(shape, generator=g) - 3.0)
    x = mag * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    x = torch.where(torch.rand(shape, generator=g) < 0.1, torch.zeros(()), x).float()
    if npix > 1:
        x[npix // 2] = 0.0
    res = (3.0 * torch.randn(shape, generator=g)).float()
    return x.numpy(), res.numpy()


def _lay(v, cs, stride, npix):
    c = v.shape[1]
    t = np.zeros((npix + TAIL, stride), f32)
    t[:npix, cs:] = np.nan
    t[:npix, :c] = v
    return t


@functools.lru_cache(maxsize=None)
def build(cid):
    """The case with its data: x / res [npix, c], the laid-out xbuf / rbuf [(npix + TAIL), stride], raw and parametrized
    parameters (fp32; bp / gp padded to cs with 1 / 0) and the float64 norm.  The data depend on (c, npix) alone."""
    k = dict(BY_ID[cid])
    c, cs, npix = k["c"], k["cs"], k["npix"]
    x, res = inputs(c, npix, 7 * c + npix)
    beta, gamma = params(c, c)
    bp, gp = parametrized(beta, 1e-6).numpy(), parametrized(gamma, 0.0).numpy()
    assert (gamma.numpy() < 2.0 ** -18).mean() > 0.05 and (gp > 0).mean() > 0.5
    xd = x.astype(np.float64)
    k.update(x=x, res=res, beta=beta.numpy(), gamma=gamma.numpy(), bp=np.ones(cs, f32), gp=np.zeros((cs, cs), f32),
             xbuf=_lay(x, cs, k["xcs"], npix), rbuf=_lay(res, cs, k["rcs"], npix),
             norm64=bp.astype(np.float64)[None, :] + (xd * xd) @ gp.astype(np.float64).T)
    k["bp"][:c] = bp
    k["gp"][:c, :c] = gp
    for v in k.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return k


def reference(k, inverse, with_res):
    """(float64 reference, per-element bound) over channels [0, c)"""
    core = k["x"].astype(np.float64) * (np.sqrt(k["norm64"]) if inverse else 1.0 / np.sqrt(k["norm64"]))
    ref = core + k["res"].astype(np.float64) if with_res else core
    return ref, ((k["c"] / 2 + 4) * np.abs(core) + np.abs(ref)) * EPS24


def new_y(k):
    """the destination: [npix + TAIL][ycs] of SENTINEL, flat (the last TAIL pixels are the guard band)"""
    return np.full((k["npix"] + TAIL) * k["ycs"], SENTINEL, f32)


# ================================================================================================ acceptance
def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def accept(k, ybuf, inverse, with_res, stats=None):
    """[] if the flat destination `ybuf` (new_y's shape) is a right answer for the case, else what is wrong with it."""
    c, cs, npix, ycs = k["c"], k["cs"], k["npix"], k["ycs"]
    fails = []
    y = np.asarray(ybuf, f32).reshape(npix + TAIL, ycs)
    sent = _bits(SENTINEL)
    if np.isnan(y).any():
        fails.append(f"{int(np.isnan(y).sum())} NaN in the destination")
    if (_bits(y[npix:]) != sent).any():
        fails.append(f"guard band written ({int((_bits(y[npix:]) != sent).sum())} elements)")
    if (_bits(y[:npix, cs:]) != sent).any():
        fails.append(f"channels [cs, ycs) written ({int((_bits(y[:npix, cs:]) != sent).sum())} elements)")
    if (_bits(y[:npix, c:cs]) != 0).any():
        fails.append("pad channels [c, cs) are not +0")
    out = y[:npix, :c]
    ref, tol = reference(k, inverse, with_res)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(out.astype(np.float64) - ref)
        ratio = np.where(err == 0, 0.0, err / tol)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    worst = float(ratio.max())
    if stats is not None:
        stats["worst"] = worst
    if not (err <= tol).all():
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        fails.append(f"{int((~(err <= tol)).sum())} of {err.size} elements outside the bound, worst |err| / bound = {worst:.3g} at "
                     f"pixel {int(i[0])} channel {int(i[1])}: got {out[i]!r}, want {ref[i]!r}")
    zero = k["x"] == 0
    want = _bits(k["res"][zero]) if with_res else np.uint32(0)
    if (_bits(out[zero]) != want).any():
        fails.append("x == 0 does not give exactly the residual / +0")
    return fails


# ================================================================================================ fp32 restatement
MUTANTS = ("no_second_pass", "second_pass_first_gamma", "drop_last_part", "gamma_transposed", "sqrt_swapped", "res_xcs",
           "stage_xcs", "write_ycs", "partial_tile_unwritten", "past_npix")
_NORMS = {}
_ORDER16 = [4 * q + e for e in range(4) for q in range(4)]  # the k order of four 16x16x4 MFMAs over one 16-channel chunk


def _chain(beta, gamma, xsq):
    """[npix, rows]: beta, then + fp32(gamma[i][j] * xsq[p][j]) for j in the kernel's order, every step rounded to fp32"""
    acc = np.repeat(beta[None, :], xsq.shape[0], 0).astype(f32)
    gt, tmp = np.ascontiguousarray(gamma.T), np.empty_like(acc)
    with np.errstate(invalid="ignore"):
        for g in range(xsq.shape[1] // 16):
            for o in _ORDER16:
                j = 16 * g + o
                np.multiply(gt[j][None, :], xsq[:, j:j + 1], out=tmp)
                acc += tmp
    return acc


def emulate(k, inverse, with_res, mutant=None, tile=None):
    """The launch restated in numpy fp32 on the case's buffers; returns the flat destination.  tile: forced pixel tile."""
    assert mutant is None or mutant in MUTANTS
    c, cs, npix, xcs, ycs, rcs = (k[n] for n in ("c", "cs", "npix", "xcs", "ycs", "rcs"))
    P = tile or tile_for(npix, cs)
    WS, NT = waves_per_16(P), cs // 16
    xs = k["xbuf"][:npix, :cs]
    xsq = xs * xs
    gamma = k["gp"].T if mutant == "gamma_transposed" else k["gp"]
    # which gamma tile and which start value every output tile gets, and whether it is written at all
    per = (NT + WS - 1) // WS
    gtile, from_beta_only, written = np.arange(NT), np.zeros(NT, bool), np.zeros(NT, bool)
    last_part = max(p for p in range(WS) if p * per < NT)
    for part in range(WS):
        for it in range(part * per, min(NT, (part + 1) * per)):
            later = (it - part * per) // IT
            written[it] = not (mutant == "drop_last_part" and NT % WS and part == last_part)
            from_beta_only[it] = mutant == "no_second_pass" and later > 0
            if mutant == "second_pass_first_gamma":
                gtile[it] = it - IT * later
    rows = (16 * gtile[:, None] + np.arange(16)[None, :]).reshape(-1)
    key = (k["id"], mutant == "gamma_transposed", tuple(gtile))  # (the chain is the same for every f, residual and tile)
    if key not in _NORMS:
        _NORMS[key] = _chain(k["bp"], gamma[rows], xsq)
    norm = _NORMS[key].copy()
    beta_only = np.repeat(from_beta_only, 16)
    norm[:, beta_only] = k["bp"][None, beta_only]
    with np.errstate(invalid="ignore", divide="ignore"):
        if mutant == "stage_xcs" and xcs > cs:  # the chunks past cs join the sum with whatever gamma holds there (say 0)
            norm = norm + (k["xbuf"][:npix, cs:] * k["xbuf"][:npix, cs:] * f32(0)).sum(1, dtype=f32)[:, None]
        f = np.sqrt(norm)
        if bool(inverse) == (mutant == "sqrt_swapped"):
            f = f32(1.0) / f
        o = xs * f
        if with_res:
            rflat = k["rbuf"].reshape(-1)
            at = np.arange(npix)[:, None] * (xcs if mutant == "res_xcs" else rcs) + np.arange(cs)[None, :]
            o = o + rflat[at]
    y = new_y(k).reshape(npix + TAIL, ycs)
    pix = npix - npix % P if mutant == "partial_tile_unwritten" else npix
    chan = np.repeat(written, 16)
    y[:pix, :cs][:, chan] = o[:pix][:, chan]
    if mutant == "write_ycs":
        y[:pix, cs:] = 0
    if mutant == "past_npix":
        y[npix:round_up(npix, P), :cs] = 0
    return y.reshape(-1)


# ================================================================================================ gamma fragments
def fragments(gp_padded):
    """[cs, cs] -> [cs / 16][cs / 16][64][4]:  [it][g][lane][e] = gamma'[16 it + lane % 16][16 g + 4 (lane / 16) + e]"""
    cs = gp_padded.shape[0]
    nt = cs // 16
    it, g, lane, e = np.meshgrid(np.arange(nt), np.arange(nt), np.arange(64), np.arange(4), indexing="ij")
    return np.ascontiguousarray(gp_padded[16 * it + lane % 16, 16 * g + 4 * (lane // 16) + e])
