"""Writes tests/golden/engine_digests.json: the SHA-256 of every output of the cases in tests/test_engine_digests_gpu.py and the
profiled launch sequences, on the GPU, at the commit that is checked out.  The cases use public entry points only, so this runs
unchanged on the commit whose bits are to be pinned:   python tools/make_engine_digests.py --commit <hash> [--out FILE]"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "licv-vqa_amd"), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit these bits belong to (recorded in the file)")
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "engine_digests.json"))
    args = ap.parse_args()
    import torch
    import test_engine_digests_gpu as T
    out = {"commit": args.commit, "sha256": {}, "launches": {}}
    for name in T.CASES:
        out["sha256"][name] = T.run_case(name)
        print(name, len(out["sha256"][name]), "outputs", flush=True)
    with torch.no_grad():
        for name, fn in T.LAUNCHES.items():
            out["launches"][name] = fn()
            print(name, len(out["launches"][name]), "launches", flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
