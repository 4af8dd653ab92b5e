"""Reading and writing the recorded sequences under tests/golden/ (seq_<name>.npz).

A sequence whose file would be larger than a committed file may be (LIMIT)
keeps its landmark snapshots (`lm`, [S+1][N][cap][6]) in pieces: seq_<name>.npz holds
every other array, parts/seq_<name>.lm<k>.npz holds lm[k].  load_seq() gives
the same arrays either way.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PARTS = os.path.join(GOLDEN, "parts")
LIMIT = 1 << 20               # a committed file's largest size


def _part(name, k):
    return os.path.join(PARTS, f"seq_{name}.lm{k}.npz")


def load_seq(name):
    """The arrays of sequence `name` as a dict."""
    d = dict(np.load(os.path.join(GOLDEN, f"seq_{name}.npz"), allow_pickle=False))
    if "lm" not in d:
        n = d["x"].shape[0]                       # one snapshot per recorded state
        d["lm"] = np.stack([np.load(_part(name, k), allow_pickle=False)["lm"] for k in range(n)])
    return d


def save_seq(name, out):
    """Write sequence `name` (the generator's side of load_seq): in one file when
    that stays within LIMIT, else with lm in pieces."""
    path = os.path.join(GOLDEN, f"seq_{name}.npz")
    np.savez_compressed(path, **out)
    if os.path.getsize(path) <= LIMIT:
        return
    out = dict(out)
    lm = np.asarray(out.pop("lm"))
    os.makedirs(PARTS, exist_ok=True)
    for k in range(lm.shape[0]):
        np.savez_compressed(_part(name, k), lm=lm[k])
    np.savez_compressed(path, **out)
