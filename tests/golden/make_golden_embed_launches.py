#!/usr/bin/env python
"""Generates tests/golden/g20_embed_launches.json: the launch sequences of the embedding forwards over tests/embed_launch_cases.py's
cases -- the fp32 forwards of CLIP, CLIP_FF, the BLIP ViT, the MED BERT and BLIP_SF, and the 16-bit forward-only passes in bf16 and
fp16 -- recorded from uniir_amd as it was BEFORE the precision rule and the fp32 launch layer were each made one ("recorded_at" in
the file: the table then pins that change, and every later one that is meant to leave the sequences alone).  The file holds ten hex
digits of the SHA-256 of every entry of every case (of the cases embed_launch_cases.LOOSE with the numbers of their temporaries
blanked, see there) and the entries themselves of embed_launch_cases.FULL.

Run:  python tests/golden/make_golden_embed_launches.py --commit <hash> [--tree <a checkout of that commit>]
      (CPU only: every op is recorded instead of launched; two runs give the same bytes.  --tree records the uniir_amd of another
      checkout with THESE cases: run on the recorded commit it reproduces the committed file byte for byte.)
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit uniir_amd was recorded at")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose uniir_amd (and oracle) is recorded")
    ap.add_argument("--out", default=os.path.join(HERE, "g20_embed_launches.json"))
    opt = ap.parse_args()
    sys.path.insert(0, os.path.abspath(opt.tree))
    sys.path.insert(0, os.path.dirname(HERE))
    import embed_launch_cases as E
    import uniir_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(uniir_amd.__file__))) == os.path.abspath(opt.tree)
    traces = {name: E.normalised(name, E.trace(name)) for name in E.NAMES}
    with open(opt.out, "w") as fh:
        fh.write('{\n "recorded_at": ' + json.dumps(opt.commit) + ',\n "loose": ' + json.dumps(list(E.LOOSE)) + ',\n "digests": {\n')
        fh.write(",\n".join(f'  {json.dumps(n)}: {json.dumps(" ".join(E.digest(e) for e in t))}' for n, t in traces.items()))
        fh.write('\n },\n "full": {\n')
        fh.write(",\n".join(f'  {json.dumps(n)}: [\n' + ",\n".join("   " + json.dumps(e, separators=(",", ":")) for e in traces[n]) + "\n  ]"
                            for n in E.FULL))
        fh.write("\n }\n}\n")
    print("g20 ok:", len(traces), "cases,", sum(len(t) - 1 for t in traces.values()), "calls,", os.path.getsize(opt.out), "bytes")


if __name__ == "__main__":
    main()
