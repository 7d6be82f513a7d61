"""Per-kernel opcode histogram of cross-compiled gfx950 assembly, and its difference between two builds of one source.
   hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only mofa_video_amd/csrc/attention.hip -o new.s   (no GPU needed)
   python tools/opcode_histogram.py old.s new.s [substring of the kernel names, default: every kernel]
Comments are stripped and instructions counted by mnemonic.  Per kernel: the instruction totals, the classes that say whether the
two builds are the same computation with the same unrolling (MFMA, v_exp, LDS reads / writes, global loads / stores: these must
be equal), and every mnemonic whose count moved."""
import collections
import re
import sys

CLASSES = [("mfma", r"v_mfma"), ("v_exp", r"v_exp"), ("lds read", r"ds_read|ds_load"), ("lds write", r"ds_write|ds_store"),
           ("global load", r"global_load|buffer_load|flat_load"), ("global store", r"global_store|buffer_store|flat_store")]


def kernels(path):
    out, name = {}, None
    for line in open(path):
        line = line.split(";")[0].split("//")[0].rstrip()
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
            out[name] = collections.Counter()
            continue
        if re.match(r"^\.Lfunc_end", line):
            name = None
        m = re.match(r"^\s+([a-z]\w+)", line)
        if m and name and not m.group(1).startswith("."):
            out[name][m.group(1)] += 1
    return out


def classes(c):
    return {cls: sum(n for op, n in c.items() if re.match(pat, op)) for cls, pat in CLASSES}


if __name__ == "__main__":
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    want = sys.argv[3] if len(sys.argv) > 3 else ""
    differ = 0
    for name in sorted(set(old) & set(new)):
        if want not in name:
            continue
        a, b = old[name], new[name]
        ca, cb = classes(a), classes(b)
        same = ca == cb
        differ += not same
        print(f"{name[:88]}\n  instructions {sum(a.values())} -> {sum(b.values())}; " +
              ", ".join(f"{k} {ca[k]}" + ("" if ca[k] == cb[k] else f" -> {cb[k]} (!)") for k in ca) +
              ("; classes equal" if same else "; CLASSES DIFFER"))
        moved = {op: (a[op], b[op]) for op in sorted(set(a) | set(b)) if a[op] != b[op]}
        if moved:
            print("  moved: " + ", ".join(f"{op} {x} -> {y}" for op, (x, y) in moved.items()))
    print(f"# kernels whose MFMA / v_exp / LDS / global-memory counts differ: {differ}")
