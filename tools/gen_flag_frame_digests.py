#!/usr/bin/env python3
"""Record tests/golden/flag_frame_digests.json: the SHA-256 of every frame of tests/flag_frames.py, per scene set-up and host
path, as the library of a checkout renders it on the GPU.  The frames and the calls come from THIS tree's tests/flag_frames.py;
the library and the binding from --root (default: this tree), so that a reference commit built beside the tree records what
the tree is then tested against:

    python tools/gen_flag_frame_digests.py --root ../parent --out tests/golden/flag_frame_digests.json
"""
import argparse
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=HERE, help="the checkout whose built library and binding render the frames")
    ap.add_argument("--out", default=os.path.join(HERE, "tests", "golden", "flag_frame_digests.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, "tests"))
    spec = importlib.util.spec_from_file_location("graft_entry_of_root", os.path.join(os.path.abspath(args.root), "__graft_entry__.py"))
    graft = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(graft)
    pkg = graft.load_package()
    gpu = pkg.load()
    import flag_frames
    out = {}
    for setup in flag_frames.SETUPS:
        for path in flag_frames.PATHS:
            out["%s/%s" % (setup, path)] = flag_frames.digests(pkg, gpu, setup, path)
            refused = sum(d.startswith("error") for v in out["%s/%s" % (setup, path)].values() for d in v)
            print("%s/%s: %d frames, %d refused calls" % (setup, path, len(out["%s/%s" % (setup, path)]), refused), flush=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", args.out, "from", gpu.path)


if __name__ == "__main__":
    main()
