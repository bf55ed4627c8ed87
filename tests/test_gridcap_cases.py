"""The grid-cap cases of tests/gridcap_cases.py are not hollow (no GPU): for every launcher row and every case

  * the case crosses the row's clamp by the launcher's own work formula -- the last sweep is partial and ends in a ragged block;
  * no element a kernel owns holds, in the reference's output, what the destination held before the launch (the file's sentinel,
    a zeroed staging buffer, the previous pass), so an element the kernel did not write cannot hide.  In-place updates by
    0.5 * tanh(lrp) are the exception: where the increment rounds away the element keeps its bits, and the check is that this is
    rare;
  * the reference's output passes the comparison the GPU test runs, and each model of a broken loop (gridcap_cases.MODELS)
    applied to it is rejected by that same comparison.

The inventory itself is checked against the sources: every clamp expression and every `grid_for(` launch of csrc/ belongs to a
row, and every row names the test that crosses it or says why none does."""
import os
import re

import numpy as np
import pytest

import gridcap_cases as gc

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "learning-based-rgb-d-image-compression_amd", "csrc")
LENIENT = ("lrp_update", "mlic_lrp_apply")  # rows whose in-place destination may keep an element's bits (a tiny increment)
CASES = gc.case_list()


@pytest.fixture(scope="module")
def refs():
    """the references that live in the GPU test files (importing them needs no GPU), and the case / oracle modules"""
    import convforms_cases as cc
    import mlic_context_cases as mc
    import refpointwise_cases as rc
    import test_gpu_mlic
    import test_gpu_stf_single
    from oracle import elic_oracle as eo

    return dict(np_slice=test_gpu_stf_single._np_slice, anchor=test_gpu_mlic._anchor, eo=eo, mc=mc, rc=rc, cc=cc)


# ---- the inventory ------------------------------------------------------------------------------------------------------------
def _sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h"))}


def test_every_clamped_launch_site_is_a_row():
    """The searches the table was built from, run again: a clamp expression or a `grid_for(` launch in a file means rows of that
    file, as many kernels as the file launches that way; a new clamped launcher without a row fails here."""
    src = _sources()
    clamp = re.compile(r"> 2048 \? 2048|g > (?:2048|4096|8192)\) g =|std::min<size_t>\([^;]*, 8192\)|g > 8192 \? 8192")
    sites = {f: len(clamp.findall(t)) for f, t in src.items() if clamp.search(t)}
    assert sites == {"entropy.hip": 3, "mlic_loop.hip": 1, "coder_abi.hip": 1, "context_attn.hip": 1, "pointwise.hip": 1,
                     "conv_mfma.hip": 1, "metrics.hip": 1, "swin.hip": 4}, sites
    # (pointwise.hip's one site is sigmoid_gate_ref's own; the rest of the file goes through grid_for(work), cap 256 * 8)
    assert "unsigned cap = 256 * 8" in src["pointwise.hip"]
    launched = set(re.findall(r"hipLaunchKernelGGL\(\(?(\w+)[^;]*?dim3\(grid_for\(", src["pointwise.hip"] + src["context_attn.hip"]))
    rows = {re.sub(r"<.*", "", r["kernel"]) for r in gc.ROWS if r["launcher"] == "grid_for"}
    assert launched == rows, (launched - rows, rows - launched)
    files = {r["file"] for r in gc.ROWS}
    assert files == set(sites), files ^ set(sites)
    for r in gc.ROWS:
        assert re.sub(r"<.*", "", r["kernel"]) in src[r["file"]], r["key"]
        assert r["crossed_by"] or r["note"], r["key"]
        if r["hook"] is None:
            assert r["crossed_by"] is None and gc.NO_HOOK in r["note"], r["key"]


def test_rows_name_tests_that_exist():
    for r in gc.ROWS:
        if r["crossed_by"]:
            path, name = r["crossed_by"].split("::")
            text = open(os.path.join(os.path.dirname(HERE), path)).read()
            assert f"def {name.split('[')[0]}(" in text, r["crossed_by"]


def test_every_hooked_row_without_a_crossing_says_why():
    left = [r["key"] for r in gc.ROWS if r["hook"] and not r["crossed_by"]]
    assert left == ["avgpool2"], left  # (with the measured cost in its note)


# ---- the cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,sweeps,rows,build", CASES, ids=[c[0] for c in CASES])
def test_case_crosses_the_cap_and_tells_a_broken_loop(cid, sweeps, rows, build, refs):
    built = build(refs)
    assert {st["row"] for st in built["stages"].values()} == set(rows)
    for sname, st in built["stages"].items():
        row = gc.BY_KEY[st["row"]]
        T = gc.threads(row)
        wk = gc.work_of(row, st["dims"])
        n_sweeps = (wk - 1) // T + 1
        ok, _, past = gc.crosses(row, st["dims"], n_sweeps)
        assert n_sweeps >= 2 and ok, (cid, sname, wk, T, past)
        if len(built["stages"]) == 1 or st["row"] != "gather_taps":
            assert n_sweeps == sweeps, (cid, sname, n_sweeps)  # (the deconv's gathers take two or three, by the phase's taps)
        # an unwritten element cannot hide
        for name, d in st["dests"].items():
            own = gc.dest_mask(d, lambda i: i >= 0)
            assert own.any()
            same = (d["want"] == d["init"]) & own
            if st["row"] in LENIENT and name in st.get("inplace", {}):
                assert same.sum() <= 0.05 * own.sum(), (cid, sname, name, int(same.sum()))
            else:
                assert not same.any(), (cid, sname, name, int(same.sum()))
            if "owner" in d:  # every loop index that owns an element is below the kernel's total
                assert int(d["owner"].max()) < gc.items_of(row, st["dims"])
        # the reference passes; every broken loop is rejected
        good = {k: d["want"] for k, d in st["dests"].items()}
        assert st["accept"](good) == [], (cid, sname)
        for model in gc.MODELS:
            bad = gc.spoil(st, model)
            if bad is None:
                assert model == "stride_short" and not st.get("inplace")
                continue
            assert st["accept"](bad), (cid, sname, model)


def test_every_row_with_a_new_test_has_a_case():
    """the rows whose crossing test is one of this table's are exactly the rows the cases above build stages for"""
    mine = {r["key"] for r in gc.ROWS if r["crossed_by"] and "past_the_grid_cap" in r["crossed_by"]}
    assert mine == {row for c in CASES for row in c[2]}
    assert len(CASES) == len({c[0] for c in CASES})
    assert {c[1] for c in CASES} == {2, 3}  # copy_channels and fill_zero also run three sweeps
