#!/usr/bin/env python
"""Generates tests/golden/g19_bert_launches.json: the launch sequences of blip_model.bert_forward / bert_backward (the MED BERT of
BLIP_FF and BLIP_SF) over tests/bert_launch_cases.py's cases, recorded from uniir_amd/blip_model.py as it was BEFORE its four copies
of the layer were folded into one forward and one backward body ("recorded_at" in the file: the table then pins that change, and
every later one that is meant to leave the sequence alone).  The file holds ten hex digits of the SHA-256 of every entry of every
case, and the entries themselves of the richest case (bert_launch_cases.FULL); to read what a digest stood for, run this script with
--out on a checkout of the recorded commit.

Run:  python tests/golden/make_golden_bert_launches.py --commit <hash of the recorded blip_model.py>
      (CPU only: every op is recorded instead of launched; two runs give the same bytes)
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import bert_launch_cases as K  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit blip_model.py was recorded at")
    ap.add_argument("--out", default=os.path.join(HERE, "g19_bert_launches.json"))
    opt = ap.parse_args()
    traces = {name: K.trace(case) for name, case in zip(K.NAMES, K.CASES)}
    # of every case one digest per entry (the whole text of 48 traces is 380 KB); of the cases K.FULL the entries too, one per line
    with open(opt.out, "w") as fh:
        fh.write('{\n "recorded_at": ' + json.dumps(opt.commit) + ',\n "digests": {\n')
        fh.write(",\n".join(f'  {json.dumps(n)}: {json.dumps(" ".join(K.digest(e) for e in t))}' for n, t in traces.items()))
        fh.write('\n },\n "full": {\n')
        fh.write(",\n".join(f'  {json.dumps(n)}: [\n' + ",\n".join("   " + json.dumps(e, separators=(",", ":")) for e in traces[n]) + "\n  ]"
                            for n in K.FULL))
        fh.write("\n }\n}\n")
    calls = sum(len(t) - 3 for t in traces.values())
    print("g19 ok:", len(traces), "cases,", calls, "calls,", os.path.getsize(opt.out), "bytes")


if __name__ == "__main__":
    main()
