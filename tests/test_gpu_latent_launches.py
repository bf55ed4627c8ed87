"""The latent stage of every family with a checkerboard slice loop does what the recorded parent commit did: same conv
launches by shape, same profiled launch count, same workspace size, same streams / outputs / y_hat bit for bit, eagerly and
through a captured graph (cases and fields: latent_launch_cases.py; the record was written by
tools/record_latent_launches.py on the commit it names and is never regenerated from the code under test)."""
import json
import os
import subprocess
import sys

import pytest

import latent_launch_cases as cases
from conftest import GOLDEN, ROOT
from gpu_utils import require_gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def record():
    with open(os.path.join(GOLDEN, "latent_launch_record.json")) as f:
        return json.load(f)


@pytest.mark.timeout(120, method="thread")
@pytest.mark.parametrize("family", list(cases.FAMILIES))
def test_same_launches_workspace_and_bits_as_the_record(record, family):
    require_gpu()
    want = record[family]
    got = cases.record_family(family)
    assert got["shape"] == want["shape"]
    assert sorted(got["calls"]) == sorted(want["calls"])
    for call, w in sorted(want["calls"].items()):
        g = got["calls"][call]
        print(f"{family} {call}: launches {g['launches']} (record {w['launches']}), workspace {g['workspace_bytes']} "
              f"(record {w['workspace_bytes']}), graphs captured {g['graphs_captured']}")
        assert g["eager_equals_graph"] and g["profiled_equals_graph"] and w["eager_equals_graph"] and w["profiled_equals_graph"], call
        for field in ("conv_log", "launches", "workspace_bytes", "graphs_captured", "sha256"):
            assert g[field] == w[field], (family, call, field)
        assert g["graphs_captured"] == 1, call


@pytest.mark.timeout(120, method="thread")
@pytest.mark.parametrize("switch", ["RGBD_NO_MEAN_CACHE", "RGBD_NO_ANCHOR_TAPS"])
def test_ab_switch_changes_no_bits(switch):
    """The switches are read once per process: a fresh child compresses the ELIC_united case at B = 2 with the switch set
    and compares its stream hashes with the record's default run."""
    require_gpu()
    env = dict(os.environ, **{switch: "1"})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "record_latent_launches.py"), "--check-streams", "ELIC_united"],
                       env=env, capture_output=True, text=True, timeout=100)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
