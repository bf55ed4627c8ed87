"""Record what the Python model classes (the six zoo classes and Spatial_aligner) show without a GPU:
tests/model_surface_cases.py has the classes and the fields.

    python tools/record_model_surface.py --commit HASH --out tests/golden/model_surface_record.json

Run it on the commit to compare AGAINST.  The committed tests/golden/model_surface_record.json is never regenerated from the
code under test: to refresh it, copy this script and tests/model_surface_cases.py into a checkout of the parent commit and run
them there.  tests/test_model_surface.py asserts the record field by field."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import model_surface_cases as cases

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", required=True, help="hash of the commit this runs on, kept in the record")
    a = ap.parse_args()
    record = {"commit": a.commit}
    for name in cases.CLASSES:
        record[name] = cases.surface(name)
        print(name, record[name]["state_dict_keys"], "keys", record[name]["upload_calls"], flush=True)
    with open(a.out, "w") as f:
        f.write("{\n" + ",\n".join(
            f" {json.dumps(k)}: " + (json.dumps(v) if isinstance(v, str) else "{\n" + ",\n".join(
                f"  {json.dumps(fk)}: {json.dumps(fv, sort_keys=True)}" for fk, fv in sorted(v.items())) + "\n }")
            for k, v in sorted(record.items())) + "\n}\n")  # one field per line
    return 0


if __name__ == "__main__":
    sys.exit(main())
