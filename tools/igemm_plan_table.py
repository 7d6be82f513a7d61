"""The pinned launch-plan table of the implicit GEMM: tests/igemm_plan_table.json.

For every row -- one mofa_igemm_args with fake, 16-byte aligned addresses and a CU count -- the table holds what
``mofa_igemm_plan`` answers: return code, tile, epilogue kind, tile counts, grid, threads, LDS, split-K and launch count.
tests/test_igemm_plan_cpu.py walks the same rows and compares, so a change of the cost model (or of any rule of
csrc/igemm_plan.h) that moves a launch to another tile shows up on the CPU.  Such a change regenerates the table on purpose:

    python tools/igemm_plan_table.py                    # the in-tree library against the table
    python tools/igemm_plan_table.py --diff OLD.so      # which rows moved since that build, old plan -> new plan, field by field
    python tools/igemm_plan_table.py [--lib OTHER.so] --write

The committed table was dumped from the commit BEFORE csrc/igemm_plan.h existed, through profiles/igemm_plan_parent_export.patch.

Rows (``rows()``; the order is part of the format).  The JSON stores the decision of every row as one letter (``CODES``: refused,
the tile, the K slices on 256x320), run-length coded per block of rows that share a shape, equal blocks once; every other field
is pinned by a SHA-256 per group over all fields of all rows:
  clip   every distinct igemm launch of one clip (profiles/r06_shape_breakdown.log: mode, stride, up, M, N, K, activation) and the
         per-rank shapes of an 8-GPU run (tools/shard_shapes_bench.py over tools/igemm_tiles_bench.py's SHAPES).  The log does not
         say which epilogue a launch had, so each shape is asked with the kinds the networks use (plain, r1, row vector, both;
         GEGLU where the log says so), with and without workspace, with and without stats, on 256 and 304 CUs.
  grid   M x N x K tiles x kinds 0-8 x workspace x CU count in all three modes (GRID_*), geometry chosen per M
  cases  every case of tests/conv_cases.py with its leading dimensions, AUTO and every forced tile
"""
import argparse
import ctypes as C
import hashlib
import itertools
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mofa_video_amd import lib as L  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "igemm_plan_table.json")
FIELDS = ("rc", "tile", "kind", "tiles_m", "tiles_n", "grid", "threads", "lds_bytes", "split", "full_tiles", "rem_tiles", "stats",
          "launches")
# fake device addresses, 16-byte aligned: the planner looks at NULL-ness and alignment only
X, W, OUT, BIAS, R1, R2, RV, WS, STATS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000, 0x90000
WS_BYTES = 256 * 256 * 320 * 4

GRID_M = (1, 255, 256, 257, 864, 7200, 8064, 64512, 460800)
GRID_N = (8, 72, 128, 256, 320, 328, 640, 1280, 2560, 3840, 10240)
GRID_NK = (1, 5, 9, 15, 45, 90, 180)
GRID_CU = (8, 64, 250, 256, 304)
# M -> (images, H, W) of a stride-1 conv / (T, HW) of the temporal conv
GRID_CONV = {1: (1, 1, 1), 255: (1, 15, 17), 256: (1, 16, 16), 257: (1, 1, 257), 864: (1, 24, 36), 7200: (1, 72, 100),
             8064: (1, 84, 96), 64512: (1, 252, 256), 460800: (50, 72, 128)}
GRID_CONVT = {1: (1, 1), 255: (3, 85), 256: (4, 64), 257: (1, 257), 864: (3, 288), 7200: (25, 288), 8064: (14, 576),
              64512: (14, 4608), 460800: (25, 9216)}


def make_args(M, N, Cin, kind=0, mode=L.MODE_PLAIN, geom=None, act=None, ws=True, stats=False, tile=L.TILE_AUTO, ldx=None, ldo=None,
              ldr=None, **over):
    """mofa_igemm_args for epilogue ``kind`` (bit 0 r1, bit 1 r2, bit 2 row vector, 8 = GEGLU pair); ``over`` sets fields last"""
    a = L.IgemmArgs()
    a.x, a.w, a.out, a.bias = X, W, OUT, BIAS
    a.M, a.N, a.Cin, a.mode, a.tile = M, N, Cin, mode, tile
    n_out = N // 2 if kind == 8 else N
    a.ldx, a.ldo = ldx or Cin, ldo or n_out
    a.act = L.ACT_GEGLU_PAIR if kind == 8 else (act or L.ACT_NONE)
    a.s_acc = a.s1 = a.s2 = 1.0
    a.stride = a.up = 1
    a.rv_div, a.rv_mul, a.rv_mod_in, a.rv_mod_out = 1, 1, 1, 1 << 30
    if kind != 8:
        if kind & 1:
            a.r1, a.ldr1 = R1, ldr or N
        if kind & 2:
            a.r2, a.ldr2 = R2, ldr or N
        if kind & 4:
            a.rowvec, a.rv_div = RV, 64 * max(M // 3200, 1)
    if geom is not None:
        for k in ("Hin", "Win", "Hout", "Wout", "stride", "up", "ksize", "T", "HW", "dil", "pad"):
            setattr(a, k, getattr(geom, k))
    if ws:
        a.workspace, a.workspace_bytes = WS, WS_BYTES
    if stats:
        a.stats = STATS
    for k, v in over.items():
        setattr(a, k, v)
    return a


class Geom:
    def __init__(self, **kw):
        self.Hin = self.Win = self.Hout = self.Wout = self.T = self.HW = self.pad = 0
        self.stride = self.up = self.dil = 1
        self.ksize = 3
        self.__dict__.update(kw)


def conv_geom(H, W, stride=1, up=1, ksize=3):
    return Geom(Hin=H, Win=W, Hout=(H * up - 1) // stride + 1, Wout=(W * up - 1) // stride + 1, stride=stride, up=up, ksize=ksize)


def _clip_rows():
    shapes = []                                                # (mode, stride, up, M, N, K, act)
    for line in open(os.path.join(ROOT, "profiles", "r06_shape_breakdown.log")):
        m = re.match(r"(gemm|conv3x3|convT3)\s+(\d)\s+(\d)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d)\s", line)
        if m:
            shapes.append((m.group(1),) + tuple(int(v) for v in m.groups()[1:]))
    src = open(os.path.join(ROOT, "tools", "igemm_tiles_bench.py")).read()      # (its import needs no GPU, but torch: read SHAPES)
    SHAPES = eval(src[src.index("SHAPES = [") + 9:src.index("\n]\n", src.index("SHAPES = [")) + 2])
    for (mode, Mg, N, Cin, epi, _, _) in SHAPES[:23]:          # tools/shard_shapes_bench.py at 8 GPUs
        if mode == "gemm":
            shapes.append(("gemm", 1, 1, Mg // 8, N, Cin, 2 if epi == "geglu" else 0))
        elif mode == "conv":
            shapes.append(("conv3x3", 1, 1, max(Mg[0] // 8, 1) * Mg[1] * Mg[2], N, 9 * Cin, 0))
        else:
            shapes.append(("convT3", 1, 1, max(Mg[1] * Mg[0] // 8, 1) * Mg[2], N, 3 * Cin, 0))
    for (mode, s, u, M, N, K, act) in sorted(set(shapes)):
        if N % 4 or K % (64 * {"gemm": 1, "conv3x3": 9, "convT3": 3}[mode]):
            continue                                           # (the 4-channel outputs run padded; not a launch of their own shape)
        if mode == "gemm":
            md, geom, Cin = L.MODE_PLAIN, None, K
        elif mode == "conv3x3":                                # M = images x Hout x Wout: 16:9 frames, the image count immaterial
            hw = next(h for h in (9 * 16 * 64 ** 2, 9 * 16 * 32 ** 2, 9 * 16 * 16 ** 2, 9 * 16 * 8 ** 2, 9 * 16 * 4 ** 2, 9 * 16, 1)
                      if M % h == 0)
            side = int(round((hw // 144) ** 0.5)) if hw >= 144 else 0
            Ho, Wo = (9 * side, 16 * side) if side else (1, 1)
            md, Cin = L.MODE_CONV3X3, K // 9
            geom = Geom(Hin=Ho * s // u, Win=Wo * s // u, Hout=Ho, Wout=Wo, stride=s, up=u)
        else:
            T = next(t for t in (25, 8, 5, 3, 2, 1) if M % t == 0)
            md, geom, Cin = L.MODE_CONVT3, Geom(T=T, HW=M // T // max(M // T // 589824, 1)), K // 3
            if M % (geom.T * geom.HW):
                geom = Geom(T=1, HW=M)
        for kind in ((8,) if act == 2 else (0, 1, 4, 5)):
            for ws in (False, True):
                for stats in ((False,) if kind == 8 else (False, True)):
                    for n_cu in (256, 304):
                        yield (f"clip {mode} s{s} u{u} M{M} N{N} K{K} | kind{kind} ws{int(ws)} stats{int(stats)} cu{n_cu}",
                               make_args(M, N, Cin, kind, md, geom, act if act not in (0, 2) else None, ws, stats), n_cu)


def _grid_rows():
    for mode in (L.MODE_PLAIN, L.MODE_CONV3X3, L.MODE_CONVT3):
        for M in GRID_M:
            for N in GRID_N:
                for nk in GRID_NK:
                    if mode == L.MODE_CONV3X3:
                        n, H, Wd = GRID_CONV[M]
                        ks = 3 if nk % 9 == 0 else 1
                        geom, Cin = conv_geom(H, Wd, ksize=ks), nk // (ks * ks) * 64
                    elif mode == L.MODE_CONVT3:
                        if nk % 3:
                            continue
                        geom, Cin = Geom(T=GRID_CONVT[M][0], HW=GRID_CONVT[M][1]), nk // 3 * 64
                    else:
                        geom, Cin = None, nk * 64
                    for kind in range(9):
                        if kind == 8 and N % 64:
                            continue
                        for ws in (False, True):
                            for n_cu in GRID_CU:
                                yield (f"grid mode{mode} M{M} N{N} nk{nk} | kind{kind} ws{int(ws)} cu{n_cu}",
                                       make_args(M, N, Cin, kind, mode, geom, ws=ws), n_cu)


def _case_rows():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import conv_cases as cc
    specs = cc.CONV_ROWS + cc.SPLIT_ROWS + cc.PIPE_OVER_ROWS + [cc.WAVE4_OVER_ROW] + cc.CONVT_ROWS + [s for K in cc.PLAIN_K for s in cc.plain_rows(K)]
    mode = {"plain": L.MODE_PLAIN, "conv": L.MODE_CONV3X3, "convt": L.MODE_CONVT3}
    for s in specs:
        for epi in cc.EPIS:
            for tile in (L.TILE_AUTO,) + tuple(cc.TILES.values()):
                for n_cu in (256, 304):
                    a = make_args(s.M, s.N, s.Cin, 1 if epi == "r1" else 0, mode[s.mode], None if s.mode == "plain" else s.geom,
                                  L.ACT_RELU if epi == "relu" else None, True, False, tile, ldx=s.Cin + 24, ldo=(s.N + 39) // 8 * 8,
                                  ldr=(s.N + 55) // 8 * 8)
                    yield f"case {s.id} {epi} | tile{tile} cu{n_cu}", a, n_cu


def rows():
    """-> (group, "block | row" description, IgemmArgs, n_cu) in table order"""
    for group, gen in (("clip", _clip_rows), ("grid", _grid_rows), ("cases", _case_rows)):
        for what, a, n_cu in gen():
            yield group, what, a, n_cu


def plan(lib, a, n_cu):
    """mofa_igemm_plan -> the tuple of FIELDS"""
    p = L.IgemmPlan()
    rc = lib.mofa_igemm_plan(C.byref(a), n_cu, C.byref(p))
    assert rc == 0 and not any(p.reserved), (rc, list(p.reserved))
    return tuple(getattr(p, f) for f in FIELDS)


def collect(lib):
    """-> [(group, description, plan)] of every row"""
    return [(group, what, plan(lib, a, n_cu)) for group, what, a, n_cu in rows()]


# The table keeps ONE LETTER per row -- the decision -- and a digest of all fields per group:
CODES = "-abcpqrstuvw"       # refused; 128x128, 192x128, 256x256; 256x320 with 1 ... 8 K slices
LEGEND = "one letter per row, run-length coded (a12 = twelve times a): " + CODES + " = refused; 128x128, 192x128, 256x256; 256x320 with 1 ... 8 K slices"


def code(t):
    rc, tile, split = t[0], t[1], t[8]
    return "-" if rc else {L.TILE_128X128: "a", L.TILE_192X128: "b", L.TILE_256X256: "c"}.get(tile) or CODES[3 + split]


def unrle(s):
    return "".join(c * int(n or 1) for c, n in re.findall(r"([-a-w])(\d*)", s))


def table(collected):
    """rows of one block (the description up to " | ") share a line of ``blocks``; equal lines are stored once"""
    blocks, rows_, sha = [], {}, {}
    for group, grp in itertools.groupby(collected, key=lambda r: r[0]):
        grp = list(grp)
        sha[group] = hashlib.sha256("".join(",".join(map(str, t)) + "\n" for _, _, t in grp).encode()).hexdigest()
        for _, blk in itertools.groupby(grp, key=lambda r: r[1].split(" | ")[0]):
            line = "".join(k + (str(n) if n > 1 else "") for k, n in ((k, len(list(v))) for k, v in itertools.groupby(code(t) for _, _, t in blk)))
            if line not in blocks:
                blocks.append(line)
            rows_.setdefault(group, []).append(blocks.index(line))
    return {"fields": list(FIELDS), "codes": LEGEND, "blocks": blocks, "rows": rows_, "sha256": sha}


def check(collected, tab):
    """-> messages: the rows whose decision is not the table's (at most 20), the groups whose other fields moved"""
    new, bad = table(collected), []
    for group, grp in itertools.groupby(collected, key=lambda r: r[0]):
        want = "".join(unrle(tab["blocks"][i]) for i in tab["rows"][group])
        grp = list(grp)
        if len(want) != len(grp):
            bad.append(f"{group}: {len(grp)} rows, the table has {len(want)}")
            continue
        moved = [f"{what}: {w} -> {code(t)}" for (_, what, t), w in zip(grp, want) if code(t) != w]
        bad += moved[:20] + ([f"{group}: {len(moved)} rows moved"] if moved else [])
        if not moved and new["sha256"][group] != tab["sha256"][group]:
            bad.append(f"{group}: tile and split of every row as pinned, but another field of some plan changed (sha256 over all fields)")
    return bad


def save(tab, path):
    with open(path, "w") as f:                                 # one block per line, 40 block indices per line
        f.write('{"fields": %s,\n "codes": %s,\n "blocks": [\n' % (json.dumps(tab["fields"]), json.dumps(tab["codes"])))
        f.write(",\n".join('  "%s"' % b for b in tab["blocks"]))
        f.write('],\n "sha256": %s,\n "rows": {' % json.dumps(tab["sha256"]))
        for i, (g, idx) in enumerate(tab["rows"].items()):
            f.write(("" if i == 0 else ",") + '\n "%s": [\n' % g)
            f.write(",\n".join("  " + ",".join(map(str, idx[k:k + 40])) for k in range(0, len(idx), 40)))
            f.write("]")
        f.write("}}\n")


def _load(path):
    lib = C.CDLL(path)
    lib.mofa_igemm_plan.argtypes = L.PROTOTYPES["mofa_igemm_plan"]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=L.LIB_PATH, help="the build of libmofa_hip.so to ask")
    ap.add_argument("--write", action="store_true", help="write tests/igemm_plan_table.json")
    ap.add_argument("--out", default=TABLE)
    ap.add_argument("--diff", default="", help="another build of the library: list every row whose plan differs, field by field")
    o = ap.parse_args()
    got = collect(_load(o.lib))
    tab = table(got)
    sizes = {g: sum(len(unrle(tab["blocks"][i])) for i in v) for g, v in tab["rows"].items()}
    print(f"{len(got)} rows {sizes}, {len(tab['blocks'])} distinct blocks")
    if o.diff:
        d = [what + ": " + ", ".join(f"{f} {x} -> {y}" for f, x, y in zip(FIELDS, t0, t1) if x != y)
             for (_, what, t0), (_, _, t1) in zip(collect(_load(o.diff)), got) if t0 != t1]
        print("\n".join(d[:200]))
        print(f"{len(d)} rows differ from {o.diff}")
    elif os.path.exists(o.out) and not o.write:
        print("\n".join(check(got, json.load(open(o.out)))) or f"every row as pinned in {o.out}")
    if o.write:
        save(tab, o.out)
        print(f"wrote {o.out}: {os.path.getsize(o.out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
