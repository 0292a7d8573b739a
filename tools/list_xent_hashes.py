#!/usr/bin/env python
"""list_xent_hashes.py -- the bits of ops.list_loss before and after the soft-target loss moved into csrc/list_loss.hip.

    python tools/list_xent_hashes.py --out profiles/list_xent_hashes_new.json
    python tools/list_xent_hashes.py --lib <libxnrs_hip.so built from the parent commit> --out profiles/list_xent_hashes_parent.json

xnrs_list_loss_fwd / _bwd share their slot scoring, slot sums, walk and join with xnrs_list_xent_*; this writes a SHA-256 of
loss, neg_scores, lse, d_up and d_table of ops.list_loss over the five shapes of tests/test_hip_list_loss.py, so that two
builds can be compared bit for bit: the two files must hold the same hashes."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libxnrs_hip.so (it may lack entry points the header declares)")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if a.lib:
        os.environ["XNRS_HIP_LIB"] = os.path.abspath(a.lib)
    import ctypes

    from xnrs_amd import hip
    if a.lib:  # bind what that build exports; the shapes below call nothing else
        probe = ctypes.CDLL(hip.LIB_PATH)
        for name in [n for n in hip.PROTOTYPES if not hasattr(probe, n)]:
            del hip.PROTOTYPES[name]
    from tests import test_hip_list_loss as LL
    out = dict(lib=os.path.basename(hip.LIB_PATH) if a.lib else "libxnrs_hip.so", build_id=hip.build_id(), shapes={})
    for shape in LL.SHAPES:
        got = LL.run(LL.case(*shape))
        out["shapes"]["x".join(map(str, shape))] = {
            k: hashlib.sha256(got[k].detach().contiguous().cpu().numpy().tobytes()).hexdigest()
            for k in ("loss", "neg_scores", "lse", "d_up", "d_table")}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out["shapes"], sort_keys=True))


if __name__ == "__main__":
    main()
