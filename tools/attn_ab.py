"""What the A/B tools (attn_temporal_long_ab.py, attn_temporal_stream_ab.py) share: two builds of libmofa_hip.so loaded into ONE
process -- ``LIBS`` = {"parent": argv[1], "new": argv[2] or the in-tree build} -- and the timing of one call on both.  The two
libraries alternate inside every round (the order flips from round to round), ROUNDS rounds of REPS launches each, events.  Per
row: the medians, the parent's run-to-run spread (max - min) / median over its rounds, and new / parent -- a ratio inside that
spread says nothing.  A process's buffer placement moves these kernels by 1-3 %, which a comparison of two processes cannot tell
from the code; this one can."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from mofa_video_amd import lib

ROUNDS, REPS = 11, 10


def load(path):
    l = C.CDLL(path)
    for name, argtypes in lib.PROTOTYPES.items():
        fn = getattr(l, name)
        fn.argtypes = argtypes
        fn.restype = lib._RESTYPE.get(name, C.c_int)
    return l


LIBS = {"parent": load(sys.argv[1]), "new": load(sys.argv[2] if len(sys.argv) > 2 else lib.LIB_PATH)}
torch.zeros(1, device="cuda")
st = lib.stream_ptr()


def timed(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e-3


def median(ts):
    return sorted(ts)[len(ts) // 2]


def ab(label, call):
    """call(library) launches once; -> whether new / parent exceeds 1 by more than the parent's spread"""
    runs = {w: (lambda l=l: call(l)) for w, l in LIBS.items()}
    for r in runs.values():
        r()
    torch.cuda.synchronize()
    ts = {"parent": [], "new": []}
    for i in range(ROUNDS):
        for w in (("parent", "new") if i % 2 == 0 else ("new", "parent")):
            ts[w].append(timed(runs[w]))
    p, n = median(ts["parent"]), median(ts["new"])
    spread = (max(ts["parent"]) - min(ts["parent"])) / p
    ratio = n / p
    flag = "" if abs(ratio - 1) <= spread else ("  SLOWER than the spread" if ratio > 1 else "  faster than the spread")
    print(f"{label:58s} parent {p * 1e6:8.1f} us  new {n * 1e6:8.1f} us  parent spread {100 * spread:4.1f} %  new / parent {ratio:5.3f}{flag}", flush=True)
    return ratio > 1 + spread


def ok(rc):
    assert rc == 0, rc
