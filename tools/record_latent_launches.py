"""Record what the latent stage (hyper synthesis -> y_hat, the checkerboard slice loop) of every family launches and
returns: tests/latent_launch_cases.py has the cases and the fields.

    python tools/record_latent_launches.py --commit HASH --out record.json     # on the commit to compare AGAINST
    python tools/record_latent_launches.py --check-streams ELIC_united         # this build's streams == the record's?

The committed tests/golden/latent_launch_record.json is never regenerated from the code under test: to refresh it, copy
this script and tests/latent_launch_cases.py into a checkout of the parent commit and run them there.
tests/test_gpu_latent_launches.py asserts the record field by field; --check-streams is what it starts in a fresh process
per A/B switch (RGBD_NO_MEAN_CACHE, RGBD_NO_ANCHOR_TAPS: read once per process, documented as changing no bits)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
RECORD = os.path.join(ROOT, "tests", "golden", "latent_launch_record.json")


def main():
    import latent_launch_cases as cases

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="write the record of every family (or of --families) here")
    ap.add_argument("--commit", default="", help="hash of the commit this runs on, kept in the record")
    ap.add_argument("--families", nargs="*", default=list(cases.FAMILIES))
    ap.add_argument("--check-streams", metavar="FAMILY", help="compress at B = 2 and compare the stream hashes with the record")
    a = ap.parse_args()
    if a.check_streams:
        import torch

        fam = a.check_streams
        with open(RECORD) as f:
            record = json.load(f)
        net = cases.make_net(fam)
        H, W = record[fam]["shape"]
        imgs = cases._images(fam, 2, H, W)
        with torch.cuda.stream(torch.cuda.Stream()):
            for _ in range(2):  # eager, then through the captured graph
                out = net.compress(*imgs)
                got = {k: cases.sha(v) for k, v in {**cases._streams("r", out["r_strings"]),
                                                    **cases._streams("d", out["d_strings"])}.items()}
                want = cases.stream_hashes(record, fam, "compress_b2")
                if got != want:
                    print(f"streams differ from the record: {got} != {want}")
                    return 1
        print("streams equal the record")
        return 0
    record = {"commit": a.commit}
    for fam in a.families:
        record[fam] = cases.record_family(fam)
        print(fam, record[fam]["shape"], {k: v["launches"] for k, v in record[fam]["calls"].items()}, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
