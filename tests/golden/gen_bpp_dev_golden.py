"""Records the CPU oracle's SQRNdbnseq tuples for the 400-nt record of tests/test_hip_bpp_dev.py (fold parity) under def.conf,
with pools of a thousand and of one, on the synthetic probabilities that test shares with the oracle: the oracle takes
40 s for them, which a GPU test that runs with every suite cannot spend.  Output: bpp_dev_400.json.gz beside this file.

    python tests/golden/gen_bpp_dev_golden.py
"""
import gzip
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import sqrn_oracle as O                                   # noqa: E402
from squarna_amd.config import ParseConfig, builtin_config            # noqa: E402
from tests.test_hip_bpp_dev import fake_bpp, parity_sequences         # noqa: E402


def main():
    names, psets = ParseConfig(builtin_config("def"))
    seq = parity_sequences()[-1]
    assert len(seq) == 400
    O.BPP_SOURCE = fake_bpp
    out = {"seq": seq, "config": "def", "folds": {}}
    for poollim in (1000, 1):
        cons, preds, cm, bm = O.SQRNdbnseq(seq, None, None, None, psets, poollim=poollim)
        out["folds"][str(poollim)] = [cons, [[d, [float(x) for x in s], [int(p) for p in ids]] for d, s, ids in preds]]
    path = os.path.join(HERE, "bpp_dev_400.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, sort_keys=True).encode())
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
