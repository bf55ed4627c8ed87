"""Pinned parity: what DESIGN.md claims about bitstream identity is ASSERTED here, against the reference's golden streams
(box-independent: tests/parity_utils.py) and at the batch shapes bench.py runs.

The north_star contract, clause by clause, per golden (tests/golden/parity_floors.json):

  * "streams"  rANS streams (y and z) byte-identical to the reference's;
  * "dbpp"     bpp (container bytes) identical: dbpp == 0 and dlen == 0;
  * "dpsnr"    |PSNR - golden| <= 1e-4 dB, per modality.

Every clause is asserted HARD for every golden unless the golden's entry lists that clause under "exceeds" -- the known
exceedances, each with its cause (the first decision that flips, the reference's own margin there, and the fp64
adjudication of tests/golden/make_fp64.py).  A listed clause keeps a recorded ceiling (the measured value; dpsnr 2 x) and
the count of parts identical before the first flip keeps its floor, so a known exceedance cannot grow silently and a NEW
one fails.  An entry that improves (a listed clause now met) passes.  A golden without an entry fails.

Also here:
  * B=8x256x256 and B=4x480x640 (the bench workloads, throughput tiles): per-image streams == B=1 calls (latency tiles),
    decoder == encoder y_hat, oracle coder re-encodes the GPU symbols to the GPU streams;
  * shared-weight clones survive a re-upload of the parent (use-after-free).

RGBD_RECORD_FLOORS=<path> dumps the measured values as JSON; tests/golden/update_floors.py turns that dump into
parity_floors.json (how the file is produced after a change of summation order, e.g. a new split-K table).
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from gpu_utils import require_gpu
from oracle import coder
from oracle import elic_oracle as eo
from parity_utils import CONTRACT_DPSNR, floors, golden_parts_identical, part_sizes

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_measured = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_measured():
    yield
    path = os.environ.get("RGBD_RECORD_FLOORS")
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(_measured, f, indent=1, sort_keys=True)


def _clause(key):
    """Contract clause a measured key belongs to (None: bookkeeping only)."""
    if key.startswith("identical"):
        return "streams"
    if key.startswith("dbpp") or key.startswith("dlen"):
        return "dbpp"
    if key.startswith("dpsnr"):
        return key  # per modality: dpsnr_r / dpsnr_d / dpsnr
    return None


def _check(case, **vals):
    """Record the measured values and hold them against the contract / the committed entry (see the module docstring)."""
    _measured[case] = {k: (bool(v) if isinstance(v, (bool, np.bool_)) else (int(v) if isinstance(v, (int, np.integer)) else
                           (v if isinstance(v, str) else float(v))))
                       for k, v in vals.items()}
    if os.environ.get("RGBD_RECORD_FLOORS") and os.environ.get("RGBD_RECORD_ONLY"):
        return  # recording run after a deliberate change of summation order: update_floors.py writes the new entries
    fl = floors().get(case)
    assert fl is not None, f"no committed entry for {case} in tests/golden/parity_floors.json"
    exceeds = set(fl.get("exceeds", []))
    for k, v in vals.items():
        if k.startswith("_") or k.startswith("flip_") or k.startswith("adj_"):
            continue
        if k.startswith("clean_parts"):
            assert v >= fl.get(k, 0), (case, k, v, fl.get(k))
            continue
        c = _clause(k)
        if c is None:
            if k.startswith("forced_"):  # decisions that differ under the reference's context: a recorded ceiling, always
                assert k in fl and v <= fl[k], (case, k, v, fl.get(k))
                continue
            if k in fl:
                assert v <= fl[k], (case, k, v, fl[k])  # (yhat_rel: float-stage ceiling)
            continue
        if c not in exceeds:  # the contract itself
            if c == "streams":
                assert bool(v), (case, k, "streams differ from the reference's and the entry does not list 'streams'")
            elif c == "dbpp":
                assert v == 0, (case, k, v, "bpp / length differs from the reference's and the entry does not list 'dbpp'")
            else:
                assert v <= CONTRACT_DPSNR, (case, k, v, f"|dPSNR| above {CONTRACT_DPSNR} dB and the entry does not list it")
        elif c != "streams":  # a known exceedance keeps its recorded ceiling
            assert k in fl, (case, k, "listed under 'exceeds' without a recorded ceiling")
            assert v <= fl[k], (case, k, v, fl[k])


FLOAT_TOL = 1e-5  # the float-stage contract (2e-5 until round 5): max |gpu - reference| / max |reference| per tensor


def _decide(x, s, table):
    sym = np.rint(np.asarray(x, np.float64)).astype(np.int64)
    idx = np.searchsorted(table[:-1].astype(np.float64), np.maximum(np.asarray(s, np.float64), np.float64(table[0])), side="left")
    return sym, idx.astype(np.int64)


def _first_flip(m, margins_name, gsym, gidx, medians=None, mods=("r", "d")):
    """Where, and by how little, the GPU's integer decisions first leave the reference's (tests/golden/make_margins.py), and
    what float64 says about it (tests/golden/make_fp64.py).

    Walks z first (a z flip changes every later context), then the y symbols in coding order (slice -> anchor / non-anchor
    -> rgb, depth).  The first differing symbol must be one the reference itself decided within a small window of a
    rounding / table boundary.  Returns
      flip_kind, flip_part, flip_ref_margin         where, and the reference's own distance to the boundary there
      flip_gpu_diff_rel                             |gpu - reference| / magnitude of the values of that part (<= FLOAT_TOL, asserted)
      flip_gpu_diff_elem                            the same difference relative to the element itself (<= 1e-3, asserted)
      flip_gpu_err64, flip_ref_err64, flip_f64_side |gpu - fp64|, |reference - fp64| at that element and which of the two
                                                    decisions float64 takes ("gpu" / "ref")
      adj_n, adj_gpu_agree, adj_ref_agree           over every near-boundary decision of the reference up to and including the
                                                    flip's part (same context for all three): how many the GPU / the
                                                    reference decide like float64."""
    path = os.path.join(GOLDEN, f"margins_{margins_name}.npz")
    assert os.path.exists(path), f"{path} is missing: the first-flip bookkeeping cannot run (tests/golden/make_margins.py)"
    mg = np.load(path)
    p64 = os.path.join(GOLDEN, f"fp64_{margins_name}.npz")
    assert os.path.exists(p64), f"{p64} is missing (tests/golden/make_fp64.py)"
    f64 = np.load(p64)
    table = m.scale_table_numpy()
    # ---- z
    if medians is not None:
        for mod, tag in enumerate(mods):
            key = f"ref_zx_{tag}"
            if key not in mg.files:
                continue
            z = m.debug_tensor("z" if len(mods) == 1 else f"z_{tag}")  # [B, N, zh, zw]
            zx = (z - medians[mod].reshape(1, -1, 1, 1)).astype(np.float32).reshape(-1)
            ref = mg[key]
            z64 = f64[f"f64_zx_{tag}"]
            bad = np.nonzero(np.rint(zx) != np.rint(ref))[0]
            if len(bad):
                i = int(bad[0])
                margin = 0.5 - abs(float(ref[i]) - float(np.rint(ref[i])))
                norm = max(float(np.abs(zx).max()), 1.0)
                diff = abs(float(zx[i]) - float(ref[i])) / norm
                elem = abs(float(zx[i]) - float(ref[i])) / max(abs(float(ref[i])), 1.0)
                assert diff <= FLOAT_TOL and elem <= 1e-3, (margins_name, "z", tag, i, float(zx[i]), float(ref[i]))
                assert margin <= mg["round_window"] * max(1.0, abs(float(ref[i]))), (margins_name, "z flip away from a boundary", margin)
                # every z decision the reference took within the window of a boundary, all modalities (one shared context: the image)
                n = ga = ra = 0
                for tg in mods:
                    r_, g_ = mg[f"ref_zx_{tg}"], (zx if tg == tag else
                                                  (m.debug_tensor(f"z_{tg}") - medians[mods.index(tg)].reshape(1, -1, 1, 1)).astype(np.float32).reshape(-1))
                    t_ = f64[f"f64_zx_{tg}"]
                    near = (0.5 - np.abs(r_ - np.rint(r_))) <= float(mg["round_window"]) * np.maximum(1.0, np.abs(r_))
                    n += int(near.sum())
                    ga += int((np.rint(g_[near]) == np.rint(t_[near])).sum())
                    ra += int((np.rint(r_[near]) == np.rint(t_[near])).sum())
                side = "gpu" if np.rint(z64[i]) == np.rint(zx[i]) else "ref"
                return {"flip_kind": f"z_{tag}", "flip_part": -1, "flip_ref_margin": margin, "flip_gpu_diff_rel": diff,
                        "flip_gpu_diff_elem": elem, "flip_gpu_err64": abs(float(zx[i]) - float(z64[i])),
                        "flip_ref_err64": abs(float(ref[i]) - float(z64[i])), "flip_f64_side": side,
                        "adj_n": n, "adj_gpu_agree": ga, "adj_ref_agree": ra}
    # ---- y, in coding order
    best = None
    for mod, tag in enumerate(mods):
        rs, ri = mg[f"ref_sym_{tag}"].astype(np.int32), mg[f"ref_idx_{tag}"].astype(np.int32)
        assert rs.shape == gsym[mod].shape, (margins_name, rs.shape, gsym[mod].shape)
        bad = np.nonzero((gsym[mod] != rs) | (gidx[mod] != ri))[0]
        if not len(bad):
            continue
        pos = int(bad[0])
        part = int(np.searchsorted(np.cumsum(mg[f"parts_{tag}"]), pos, side="right"))
        if best is None or (part, mod) < best[:2]:
            best = (part, mod, tag, pos, "index" if gidx[mod][pos] != ri[pos] else "round")
    if best is None:
        return {}
    part, mod, tag, pos, kind = best
    xg, sg = m.debug_floats(mod)
    nb = mg[f"nb_pos_{tag}"]
    j = int(np.searchsorted(nb, pos))
    assert j < len(nb) and nb[j] == pos, (margins_name, f"first differing symbol ({tag} part {part} pos {pos}) was not near a "
                                          "boundary in the reference's own floats")
    xr, sr = float(mg[f"nb_x_{tag}"][j]), float(mg[f"nb_s_{tag}"][j])
    x64, s64 = float(f64[f"f64_nb_x_{tag}"][j]), float(f64[f"f64_nb_s_{tag}"][j])
    ends = np.cumsum(mg[f"parts_{tag}"])
    lo, hi = (int(ends[part - 1]) if part else 0), int(ends[part])
    if kind == "round":  # magnitude of the values of this part (not of the whole tensor, scales included)
        norm = max(float(np.abs(xg[lo:hi]).max()), 1.0)
        margin = 0.5 - abs(xr - float(np.rint(xr)))
        diff, elem = abs(float(xg[pos]) - xr) / norm, abs(float(xg[pos]) - xr) / max(abs(xr), 1.0)
        e_g, e_r = abs(float(xg[pos]) - x64), abs(xr - x64)
        side = "gpu" if np.rint(x64) == gsym[mod][pos] else "ref"
    else:
        norm = max(float(np.abs(sg[lo:hi]).max()), 1.0)
        margin = float(np.abs(sr / table[:-1] - 1.0).min())
        diff, elem = abs(float(sg[pos]) - sr) / norm, abs(float(sg[pos]) - sr) / max(abs(sr), float(table[0]))
        e_g, e_r = abs(float(sg[pos]) - s64), abs(sr - s64)
        side = "gpu" if _decide([0.0], [s64], table)[1][0] == gidx[mod][pos] else "ref"
    assert diff <= FLOAT_TOL and elem <= 1e-3, (margins_name, kind, tag, pos, diff, elem)
    # adjudication over the near-boundary decisions taken under the same context: parts before the flip's (both modalities) and
    # the flip's own part (its symbols are decided in parallel from one context)
    n = ga = ra = 0
    for mod2, tag2 in enumerate(mods):
        nb2 = mg[f"nb_pos_{tag2}"]
        ends2 = np.cumsum(mg[f"parts_{tag2}"])
        last = part if (mod2 <= mod) else part - 1  # coding order inside a part index: rgb before depth
        if last < 0:
            continue
        sel = nb2 < int(ends2[last])
        if not sel.any():
            continue
        pp = nb2[sel]
        s64v, i64v = _decide(f64[f"f64_nb_x_{tag2}"][sel], f64[f"f64_nb_s_{tag2}"][sel], table)
        rs2, ri2 = mg[f"ref_sym_{tag2}"].astype(np.int64)[pp], mg[f"ref_idx_{tag2}"].astype(np.int64)[pp]
        n += len(pp)
        ga += int(((gsym[mod2][pp] == s64v) & (gidx[mod2][pp] == i64v)).sum())
        ra += int(((rs2 == s64v) & (ri2 == i64v)).sum())
    return {"flip_kind": f"{kind}_{tag}", "flip_part": 2 * part + mod, "flip_ref_margin": margin, "flip_gpu_diff_rel": diff,
            "flip_gpu_diff_elem": elem, "flip_gpu_err64": e_g, "flip_ref_err64": e_r, "flip_f64_side": side,
            "adj_n": n, "adj_gpu_agree": ga, "adj_ref_agree": ra}


def _model(name, sd):
    import rgbd_amd

    m = rgbd_amd.modelZoo[name](config=rgbd_amd.model_config(), channel=3 if name == "ELIC" else 4).eval()
    m.load_state_dict(sd, strict=True)
    assert m.update(force=True)
    return m.to("cuda")


@pytest.fixture(scope="module")
def net(synth_sd):
    require_gpu()
    return _model("ELIC_united", synth_sd)


@pytest.fixture(scope="module")
def gc(kat):
    return coder.Tables(kat["gc_cdf"], kat["gc_sizes"], kat["gc_offsets"])


def _symbols(m, mods=2):
    gsym, gidx = {}, {}
    for mod in range(mods):
        gsym[mod], gidx[mod] = m.debug_symbols(mod)
    return gsym, gidx


def _pad_inputs(B, H, W, cid, smooth=False):
    from rgbd_amd import synth

    r, d = synth.synthetic_batch(B, H, W, config_id=cid, smooth=smooth)
    r, d = torch.from_numpy(r), torch.from_numpy(d)
    return r, d, eo.pad_replicate0(r), eo.pad_replicate0(d)


# ---- end-to-end ELIC_united against every model golden ----------------------------------------------------------------
@pytest.fixture(scope="module")
def net_tl():
    """ELIC_united with the trained_like synthetic weights (the coder's realistic operating point, ~3.6 bpp)."""
    require_gpu()
    from rgbd_amd import synth

    return _model("ELIC_united", synth.synthetic_state_dict(0, recipe="trained_like"))


def test_elic_united_trained_like_vs_reference_golden(net_tl, gc):
    """The bench's image shape (480x640, padded to 512x640) with the trained_like weights against the reference's run of
    the same case (tests/golden/make_golden.py --only-e)."""
    _vs_golden(net_tl, gc, "e_480x640_tl")


def test_elic_united_high_rate_vs_reference_golden(gc):
    """The high_rate synthetic weights (98 % of the symbols on scale-table rows of 300 ... 3000 entries: the rows the decoder
    searches through its coarse first level) against the reference's run of the same case (make_golden.py --only-hr)."""
    from rgbd_amd import synth

    require_gpu()
    _vs_golden(_model("ELIC_united", synth.synthetic_state_dict(0, recipe="high_rate")), gc, "i_128x192_hr")


@pytest.mark.parametrize("name", ["a_128x192", "b_100x150", "c_b2_128x128", "d_256x256", "f_480x640_stress"])
def test_elic_united_vs_reference_golden(net, gc, name):
    """f_480x640_stress: the bench's own operating point (c3's image shape with the stress recipe the bench runs)."""
    _vs_golden(net, gc, name)


@pytest.mark.parametrize("name,seed,recipe", [("g_256x256_s1", 1, None), ("h_256x256_s2", 2, None), ("j_192x256_s3", 3, None),
                                              ("k_200x300_tl_s4", 4, "trained_like"), ("l_b2_192x256_s5", 5, None),
                                              ("m_256x320_smooth_s7", 7, None), ("p_480x640_s10", 10, None)])
def test_elic_united_other_weight_seeds_vs_reference_golden(gc, name, seed, recipe):
    """The flip census seeds (profiles/r02_flip_census.json was against the box's oracle) against the reference itself.
    j_192x256_s3 and k_200x300_tl_s4 (round 5) are HELD-OUT cases: image sizes (the second one needs padding, -> 256 x 320, and
    runs the trained-like weights) and weight seeds nothing had seen when the reference-arithmetic path was written; only their
    layer shapes were measured afterwards (tools/refarith/discover.py --add united:H:W:B).  l_b2_192x256_s5 is the reference's
    batched calling convention (one stream per batch of two) at a held-out size and seed; m_256x320_smooth_s7 codes spatially
    correlated images (every other golden codes uniform noise); p_480x640_s10 is the bench's own image shape with another
    weight seed and other images."""
    from rgbd_amd import synth

    require_gpu()
    sd = synth.synthetic_state_dict(seed) if recipe is None else synth.synthetic_state_dict(seed, recipe=recipe)
    _vs_golden(_model("ELIC_united", sd), gc, name)


def _vs_golden(net, gc, name):
    g = load_golden(name)
    B, H, W = int(g["B"]), int(g["H"]), int(g["W"])
    r, d, rp, dp = _pad_inputs(B, H, W, int(g["config_id"]), smooth="smooth" in g)
    net.per_image_streams = False  # the reference's format (one y-stream per modality for the batch)
    net.set_debug_floats(True)
    try:
        out = net.compress(rp.cuda(), dp.cuda())
    finally:
        net.set_debug_floats(False)
    assert tuple(out["shape"]) == tuple(g["shape"])
    # z-streams: identical to the reference's unless a z value sits on a rounding boundary (d_256x256: one depth symbol)
    z_same = all(out[key][1][i] == g[f"{m}_z{i}"].tobytes() for m, key in (("r", "r_strings"), ("d", "d_strings"))
                 for i in range(B))
    gsym, gidx = _symbols(net)
    h, w = rp.shape[-2] // 16, rp.shape[-1] // 16
    clean, total = golden_parts_identical(gsym, gidx, {0: g["r_y"].tobytes(), 1: g["d_y"].tobytes()}, gc,
                                          part_sizes(net.slice_ch, h, w, B))
    same = out["r_strings"][0][0] == g["r_y"].tobytes() and out["d_strings"][0][0] == g["d_y"].tobytes()
    assert same == (clean == total)
    # (before decompress(): it reuses the workspace the encoder's debug tensors live in)
    flip = {} if (same and z_same) else _first_flip(net, name, gsym, gidx, medians=net.eb_medians_numpy())
    rec = net.decompress(out["r_strings"], out["d_strings"], out["shape"])
    xr, xd = rec["x_hat"]["r"].cpu()[..., :H, :W], rec["x_hat"]["d"].cpu()[..., :H, :W]
    vals = {"clean_parts_vs_golden": clean, "identical_streams": same, "identical_z": z_same,
            "dpsnr_r": abs(eo.psnr(xr, r) - g["psnr"][0]), "dpsnr_d": abs(eo.psnr(xd, d) - g["psnr"][1]),
            "dlen_r": abs(len(out["r_strings"][0][0]) - g["r_y"].shape[0]),
            "dlen_d": abs(len(out["d_strings"][0][0]) - g["d_y"].shape[0])}
    if "bpp" in g:
        bpp = [len(eo.container_bytes(H, W, out["shape"], out[k])) * 8.0 / (H * W) for k in ("r_strings", "d_strings")]
        vals["dbpp_r"], vals["dbpp_d"] = abs(bpp[0] - g["bpp"][0]), abs(bpp[1] - g["bpp"][1])
    vals.update(flip)
    print(name, vals)
    _check(name, **vals)


# ---- Bi-CEE alone (BASELINE config 4) -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c4_16x16", "c4_b2_8x12"])
def test_bicee_vs_reference_golden(net, gc, name):
    from rgbd_amd import synth

    g = np.load(os.path.join(GOLDEN, f"bicee_{name}.npz"))
    B, h, w = int(g["B"]), int(g["h"]), int(g["w"])
    yr, hr, yd, hd = [torch.from_numpy(a).cuda() for a in synth.synthetic_latents(B, h, w, 320, int(g["seed"]))]
    net.per_image_streams = False
    net.set_debug_floats(True)
    try:
        sr, sdp = net.compress_united(yr, hr, yd, hd)
    finally:
        net.set_debug_floats(False)
    gsym, gidx = _symbols(net)
    clean, total = golden_parts_identical(gsym, gidx, {0: g["r_y"].tobytes(), 1: g["d_y"].tobytes()}, gc,
                                          part_sizes(net.slice_ch, h, w, B))
    same = sr[0] == g["r_y"].tobytes() and sdp[0] == g["d_y"].tobytes()
    assert same == (clean == total)
    flip = {} if same else _first_flip(net, "bicee_" + name, gsym, gidx)
    yhat_r, yhat_d = net.decompress_united(sr[0], hr, sdp[0], hd)
    vals = {"clean_parts_vs_golden": clean, "identical_streams": same,
            "dlen_r": abs(len(sr[0]) - g["r_y"].shape[0]), "dlen_d": abs(len(sdp[0]) - g["d_y"].shape[0])}
    vals.update(flip)
    if same:  # then y_hat is the reference's, up to the float tolerance of the means
        vals["yhat_rel"] = max(float(np.abs(yhat_r.cpu().numpy() - g["yhat_r"]).max() / np.abs(g["yhat_r"]).max()),
                               float(np.abs(yhat_d.cpu().numpy() - g["yhat_d"]).max() / np.abs(g["yhat_d"]).max()))
    print(name, vals)
    _check("bicee_" + name, **vals)


# ---- the other model families ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,seed", [("128x192", 0), ("o_192x256_s9", 9)])
def test_r2d_vs_reference_golden(gc, case, seed):
    """o_192x256_s9 (round 5): the held-out case of this model family (tools/refarith/discover.py --add r2d:192:256:1)."""
    from rgbd_amd import synth

    require_gpu()
    m = _model("ELIC_united_R2D", synth.synthetic_state_dict(seed, model="ELIC_united_R2D"))
    g = np.load(os.path.join(GOLDEN, f"r2d_{case}.npz"))
    H, W = int(g["H"]), int(g["W"])
    r, d = synth.synthetic_batch(1, H, W, config_id=int(g["config_id"]))
    out = m.compress(torch.from_numpy(r).cuda(), torch.from_numpy(d).cuda())
    gsym, gidx = _symbols(m)
    clean, total = golden_parts_identical(gsym, gidx, {0: g["r_y"].tobytes(), 1: g["d_y"].tobytes()}, gc,
                                          part_sizes(m.slice_ch, H // 16, W // 16))
    same = (out["r_strings"][0][0] == g["r_y"].tobytes() and out["d_strings"][0][0] == g["d_y"].tobytes() and
            out["r_strings"][1][0] == g["r_z0"].tobytes() and out["d_strings"][1][0] == g["d_z0"].tobytes())
    rec = m.decompress(out["r_strings"], out["d_strings"], out["shape"])
    xr, xd = rec["x_hat"]["r"].cpu(), rec["x_hat"]["d"].cpu()
    vals = {"clean_parts_vs_golden": clean, "identical_streams": same,
            "dpsnr_r": abs(eo.psnr(xr, torch.from_numpy(r)) - g["psnr"][0]),
            "dpsnr_d": abs(eo.psnr(xd, torch.from_numpy(d)) - g["psnr"][1])}
    print("r2d", case, vals)
    _check("r2d_" + case, **vals)


@pytest.mark.parametrize("case,seed", [("c1_256x256", 0), ("n_192x256_s8", 8)])
def test_elic_single_vs_reference_golden(gc, case, seed):
    """c1_256x256: BASELINE config 1.  n_192x256_s8 (round 5): a held-out single-modal case -- image size and weight seed chosen after
    the fact, its layer shapes measured with tools/refarith/discover.py --add single:192:256:1."""
    from rgbd_amd import synth

    require_gpu()
    m = _model("ELIC", synth.synthetic_state_dict(seed, model="ELIC"))
    g = np.load(os.path.join(GOLDEN, f"elic_{case}.npz"))
    H, W = int(g["H"]), int(g["W"])
    r, _ = synth.synthetic_batch(1, H, W, config_id=int(g["config_id"]))
    x = torch.from_numpy(r)
    m.set_debug_floats(True)
    out = m.compress(x.cuda())
    m.set_debug_floats(False)
    gsym, gidx = _symbols(m, 1)
    clean, total = golden_parts_identical(gsym, gidx, {0: g["y_stream"].tobytes()}, gc, part_sizes(m.slice_ch, H // 16, W // 16),
                                          modalities=1)
    same = out["strings"][0][0] == g["y_stream"].tobytes() and out["strings"][1][0] == g["z0"].tobytes()
    flip = {} if same else _first_flip(m, "elic_" + case, gsym, gidx, medians=m.eb_medians_numpy(), mods=("r",))
    rec = m.decompress(out["strings"], out["shape"])
    vals = {"clean_parts_vs_golden": clean, "identical_streams": same,
            "dpsnr": abs(eo.psnr(rec["x_hat"].cpu().clamp(0, 1), x) - g["psnr"][0]),
            "dlen": abs(len(out["strings"][0][0]) - g["y_stream"].shape[0])}
    vals.update(flip)
    print("elic single", case, vals)
    _check("elic_" + case, **vals)


def test_stf_vs_reference_golden(kat):
    _stf_vs_golden(kat, "c5_256x256")


@pytest.mark.parametrize("case", ["q_b2_256x320", "r_320x256_s11"])
def test_stf_heldout_vs_reference_golden(kat, case):
    """STF_united off the square (make_golden.py --only-stf): B=2 at 256x320, the batch coded into one y stream per modality,
    and 320x256 with weight seed 11, both on images no other fixture uses."""
    _stf_vs_golden(kat, case)


def _stf_vs_golden(kat, case):
    from rgbd_amd import synth

    require_gpu()
    g = np.load(os.path.join(GOLDEN, f"stf_{case}.npz"))
    B, H, W = int(g["B"]), int(g["H"]), int(g["W"])
    sd = synth.synthetic_state_dict(int(g["seed"]) if "seed" in g.files else 0, model="STF_united")
    m = _model("STF_united", sd)
    r, d = synth.synthetic_batch(B, H, W, config_id=int(g["config_id"]))
    m.set_debug_floats(True)
    out = m.compress(torch.from_numpy(r).cuda(), torch.from_numpy(d).cuda())
    m.set_debug_floats(False)
    gsym, gidx = _symbols(m)
    gc5 = coder.Tables(kat["gc_cdf"], kat["gc_sizes"], kat["gc_offsets"])  # the Gaussian table does not depend on the model
    clean, total = golden_parts_identical(gsym, gidx, {0: g["r_y"].tobytes(), 1: g["d_y"].tobytes()}, gc5,
                                          part_sizes(m.slice_ch, H // 16, W // 16, B))
    same = out["r_strings"][0][0] == g["r_y"].tobytes() and out["d_strings"][0][0] == g["d_y"].tobytes()
    z_same = all(out[key][1][i] == g[f"{t}_z{i}"].tobytes() for t, key in (("r", "r_strings"), ("d", "d_strings"))
                 for i in range(B))
    flip = {} if (same and z_same) else _first_flip(m, "stf_" + case, gsym, gidx, medians=m.eb_medians_numpy())
    rec = m.decompress(out["r_strings"], out["d_strings"], out["shape"])
    xr, xd = rec["x_hat"]["r"].cpu(), rec["x_hat"]["d"].cpu()
    vals = {"clean_parts_vs_golden": clean, "identical_streams": same, "identical_z": z_same,
            "dpsnr_r": abs(eo.psnr(xr, torch.from_numpy(r)) - g["psnr"][0]),
            "dpsnr_d": abs(eo.psnr(xd, torch.from_numpy(d)) - g["psnr"][1]),
            "dlen_r": abs(len(out["r_strings"][0][0]) - g["r_y"].shape[0])}
    vals.update(flip)
    print("stf", case, vals)
    _check("stf_" + case, **vals)


# ---- teacher forcing: every part of the goldens that are NOT identical, under the reference's context ------------------------
def _forced_census(m, margins_name, run, medians=None):
    """Round-4 review, item 2.  A first flip changes every later context, so the parts behind it were never compared with the
    reference.  Here the engine rebuilds z_hat / y_hat after the z stage and after each coding part from the REFERENCE's
    symbols (rgbd_elic_set_forced_symbols; tests/golden/margins_*.npz), while its decisions still come from its own floats:
    all 20 parts (and z) are then decided under exactly the context the reference decided them under
    (models/elic_united.py:265-348), and every decision that differs is counted.  Each one must be a decision the reference
    itself took within its window of a boundary (the near-boundary list), with the GPU's float within FLOAT_TOL of the
    reference's there."""
    mg = np.load(os.path.join(GOLDEN, f"margins_{margins_name}.npz"))
    tags = ("r", "d")
    for mod, tag in enumerate(tags):
        zs = mg[f"ref_zsym_{tag}"].astype(np.int32) if (medians is not None and f"ref_zsym_{tag}" in mg.files) else None
        m.set_forced_symbols(mod, mg[f"ref_sym_{tag}"].astype(np.int32), zs)
    m.set_debug_floats(True)
    try:
        run()
        gsym, gidx = _symbols(m)
        floats = [m.debug_floats(mod) for mod in range(2)]
        zt = [m.debug_tensor(f"z_{tag}") for tag in tags] if medians is not None else None
    finally:
        m.set_debug_floats(False)
        for mod in range(2):
            m.set_forced_symbols(mod)
    table = m.scale_table_numpy()
    flips = decisions = zflips = zdec = 0
    dirty = set()
    worst = 0.0
    for mod, tag in enumerate(tags):
        rs, ri = mg[f"ref_sym_{tag}"].astype(np.int32), mg[f"ref_idx_{tag}"].astype(np.int32)
        assert rs.shape == gsym[mod].shape
        bs, bi = gsym[mod] != rs, gidx[mod] != ri
        decisions += 2 * rs.size  # one rounding and one table-row decision per element
        flips += int(bs.sum()) + int(bi.sum())
        bad = np.nonzero(bs | bi)[0]
        if not len(bad):
            continue
        ends = np.cumsum(mg[f"parts_{tag}"])
        nb = mg[f"nb_pos_{tag}"]
        j = np.searchsorted(nb, bad)
        assert (j < len(nb)).all() and (nb[np.minimum(j, len(nb) - 1)] == bad).all(), \
            (margins_name, tag, "a forced-context decision differs where the reference was NOT near a boundary", bad[:8])
        xg, sg = floats[mod]
        for pos, jj in zip(bad, j):
            part = int(np.searchsorted(ends, pos, side="right"))
            dirty.add((part, mod))
            lo, hi = (int(ends[part - 1]) if part else 0), int(ends[part])
            if bs[pos]:
                d = abs(float(xg[pos]) - float(mg[f"nb_x_{tag}"][jj])) / max(float(np.abs(xg[lo:hi]).max()), 1.0)
            else:
                d = abs(float(sg[pos]) - float(mg[f"nb_s_{tag}"][jj])) / max(float(np.abs(sg[lo:hi]).max()), 1.0)
            worst = max(worst, d)
            assert d <= FLOAT_TOL, (margins_name, tag, int(pos), d)
    if zt is not None:
        for mod, tag in enumerate(tags):
            if f"ref_zsym_{tag}" not in mg.files:
                continue
            zx = (zt[mod] - medians[mod].reshape(1, -1, 1, 1)).astype(np.float32).reshape(-1)
            zb = np.rint(zx) != mg[f"ref_zsym_{tag}"].astype(np.float32)
            zdec += zx.size
            zflips += int(zb.sum())
            for i in np.nonzero(zb)[0]:
                ref = float(mg[f"ref_zx_{tag}"][i])
                assert 0.5 - abs(ref - float(np.rint(ref))) <= float(mg["round_window"]) * max(1.0, abs(ref)), (margins_name, "z", tag, int(i))
                worst = max(worst, abs(float(zx[i]) - ref) / max(float(np.abs(zx).max()), 1.0))
    nparts = 2 * len(mg["parts_r"])
    return {"forced_flips": flips, "forced_z_flips": zflips, "_forced_decisions": decisions + zdec,
            "_forced_parts": nparts, "_forced_parts_clean": nparts - len(dirty), "_forced_worst_rel": worst,
            "_forced_flips_per_million": 1e6 * (flips + zflips) / max(decisions + zdec, 1)}


@pytest.mark.parametrize("name", ["c4_b2_8x12"])
def test_teacher_forced_bicee(net, name):
    from rgbd_amd import synth

    g = np.load(os.path.join(GOLDEN, f"bicee_{name}.npz"))
    B, h, w = int(g["B"]), int(g["h"]), int(g["w"])
    yr, hr, yd, hd = [torch.from_numpy(a).cuda() for a in synth.synthetic_latents(B, h, w, 320, int(g["seed"]))]
    net.per_image_streams = False
    vals = _forced_census(net, "bicee_" + name, lambda: net.compress_united(yr, hr, yd, hd))
    print("forced bicee", name, vals)
    _check("forced_bicee_" + name, **vals)


def test_teacher_forced_identical_golden_is_a_no_op(net):
    """On a golden whose streams are identical, forcing the reference's symbols must change nothing: no decision differs and
    the stream is still the reference's (the hook rebuilds y_hat as symbol + mean, exactly what the encoder had written)."""
    g = load_golden("d_256x256")
    r, d, rp, dp = _pad_inputs(1, 256, 256, int(g["config_id"]))
    net.per_image_streams = False
    out = {}
    vals = _forced_census(net, "d_256x256", lambda: out.update(net.compress(rp.cuda(), dp.cuda())), medians=net.eb_medians_numpy())
    assert vals["forced_flips"] == 0 and vals["forced_z_flips"] == 0, vals
    assert out["r_strings"][0][0] == g["r_y"].tobytes() and out["d_strings"][0][0] == g["d_y"].tobytes()


def test_teacher_forced_stf():
    from rgbd_amd import synth

    require_gpu()
    m = _model("STF_united", synth.synthetic_state_dict(0, model="STF_united"))
    g = np.load(os.path.join(GOLDEN, "stf_c5_256x256.npz"))
    r, d = synth.synthetic_batch(1, 256, 256, config_id=int(g["config_id"]))
    vals = _forced_census(m, "stf_c5_256x256", lambda: m.compress(torch.from_numpy(r).cuda(), torch.from_numpy(d).cuda()),
                          medians=m.eb_medians_numpy())
    print("forced stf", vals)
    _check("forced_stf_c5_256x256", **vals)


# ---- the bench's batch shapes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,cid", [(8, 256, 256, 2), (4, 480, 640, 3), (16, 480, 640, 3), (32, 256, 256, 2)])
def test_bench_shapes_batch_and_tile_invariance(net, gc, B, H, W, cid):
    """bench.py's workloads (c2: 8x256x256, c3: 4x480x640 -> 512x640, and c3's engine-call shape since round 5: four steps =
    16 images per call for c3, 32 for c2, bench.py --steps-per-call) in the tile mode the bench times (throughput tiles)
    against B=1 calls with the latency tiles: the per-image streams, the decoder's y_hat and x_hat must not move by a bit."""
    r, d, rp, dp = _pad_inputs(B, H, W, cid)
    rp, dp = rp.cuda(), dp.cuda()
    net.per_image_streams = True
    try:
        net.set_tile_mode("throughput")
        out = net.compress(rp, dp)
        assert len(out["r_strings"][0]) == B and len(out["d_strings"][0]) == B and len(out["r_strings"][1]) == B
        gsym, gidx = _symbols(net)
        T = gsym[0].shape[0] // B
        for mod, key in ((0, "r_strings"), (1, "d_strings")):  # integer stage at full size: oracle coder == GPU coder
            for i in range(B):
                assert coder.rans_encode(gsym[mod][i * T:(i + 1) * T], gidx[mod][i * T:(i + 1) * T], gc) == out[key][0][i]
        yhat = [net.debug_tensor("yhat_r").copy(), net.debug_tensor("yhat_d").copy()]
        rec = net.decompress(out["r_strings"], out["d_strings"], out["shape"])
        assert np.array_equal(net.debug_tensor("yhat_r"), yhat[0]) and np.array_equal(net.debug_tensor("yhat_d"), yhat[1])
        net.set_tile_mode("latency")
        for i in range(B):
            one = net.compress(rp[i:i + 1], dp[i:i + 1])
            for key in ("r_strings", "d_strings"):
                assert one[key][0][0] == out[key][0][i], (key, i)
                assert one[key][1][0] == out[key][1][i], (key, i)
            rec1 = net.decompress(one["r_strings"], one["d_strings"], one["shape"])
            assert torch.equal(rec1["x_hat"]["r"][0], rec["x_hat"]["r"][i]) and torch.equal(rec1["x_hat"]["d"][0], rec["x_hat"]["d"][i])
        # the same batch in the latency tiles: every bit the same (tile choice is a pure speed matter)
        out_l = net.compress(rp, dp)
        assert out_l["r_strings"] == out["r_strings"] and out_l["d_strings"] == out["d_strings"]
    finally:
        net.per_image_streams = False
        net.set_tile_mode("latency")


# ---- shared-weight clones ------------------------------------------------------------------------------------------------------
def test_clone_survives_parent_reupload(synth_sd):
    """a parent re-upload used to free the buffers its clones point at.  Device buffers are reference-counted
    now and a clone re-clones itself when its parent has moved on."""
    import rgbd_amd
    from rgbd_amd import RgbdError, synth

    require_gpu()
    pool = rgbd_amd.CodecPool(synth_sd, config=rgbd_amd.model_config(), workers=2, device="cuda", per_image_streams=True)
    r, d = synth.synthetic_batch(1, 128, 128, config_id=21)
    rgb, depth = torch.from_numpy(r).cuda(), torch.from_numpy(d).cuda()
    before = pool.nets[1].compress(rgb, depth)
    assert pool.nets[0].update(force=True)      # parent: tables rebuilt, weights re-uploaded on the next call
    mid = pool.nets[1].compress(rgb, depth)      # the clone follows the parent (fresh clone of the new generation)
    assert mid["r_strings"] == before["r_strings"] and mid["d_strings"] == before["d_strings"]
    rec = pool.nets[1].decompress(mid["r_strings"], mid["d_strings"], mid["shape"])
    ref = pool.nets[0].decompress(mid["r_strings"], mid["d_strings"], mid["shape"])
    assert torch.equal(rec["x_hat"]["r"], ref["x_hat"]["r"]) and torch.equal(rec["x_hat"]["d"], ref["x_hat"]["d"])
    # new weights on the parent reach the clone
    sd2 = synth.synthetic_state_dict(1)
    pool.nets[0].load_state_dict(sd2)
    pool.nets[0].update(force=True)
    a = pool.nets[0].compress(rgb, depth)
    b = pool.nets[1].compress(rgb, depth)
    assert a["r_strings"] == b["r_strings"] and a["r_strings"] != before["r_strings"]
    with pytest.raises(RgbdError):
        pool.nets[1].update(force=True)
    # a clone outlives its parent's python object being re-uploaded again while it is mid-use
    pool.nets[0].update(force=True)
    pool.nets[0].compress(rgb, depth)
    c = pool.nets[1].compress(rgb, depth)
    assert c["r_strings"] == a["r_strings"]
    pool.close()
