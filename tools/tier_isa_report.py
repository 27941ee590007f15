"""What the compiler made of the tier kernels' loads (no GPU): csrc/direct.hip is compiled device-only to gfx950 assembly with the
Makefile's flags, and for every k_nd_tier instantiation the script prints

    global loads                        global_load_* instructions
    full waits                          s_waitcnt with vmcnt(0): the wave stops until EVERY vector-memory load it has in flight is back
    full wait directly after a load     a load whose very next instruction is such a wait: a round trip nothing was overlapped with
    VGPRs, scratch bytes                from the kernel's own resource comments (budget: 128 VGPRs, scratch 0)

A gather that the source writes as `if (idx >= 0) v += x[idx]` per child comes out as one predicated block per child -- load, full wait,
add -- i.e. one serial round trip per child; the same gather from a clamped index with the sum taken by a select keeps the loads back to
back behind ONE counted wait (nd_tier.h, pull_request / pull_sum). This report is how that was found and how it is kept.

    python tools/tier_isa_report.py                  the table
    python tools/tier_isa_report.py --pairs          ... and, per kernel, every load + full wait pair with its source line (-g1 build)
    python tools/tier_isa_report.py --asm out.s      keep the assembly
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "large-steps-pytorch_amd", "csrc")
NAME = re.compile(r"^_ZN2ls9k_nd_tierILi(\d+)ELb([01])ELi(\d+)ELb([01])EEEv")


def makefile_flags():
    """CXXFLAGS of csrc/Makefile with $(ARCH) = gfx950"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", "gfx950").split()


def assembly(extra=()):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "direct.s")
        subprocess.run([hipcc] + makefile_flags() + list(extra) + ["--cuda-device-only", "-S", "direct.hip", "-o", out], cwd=CSRC, check=True)
        return open(out).read()


def tier_kernels(asm):
    """{(K, up, waves, nt): [instruction lines of the kernel's body, resource comments included]}"""
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^(\S+):\s*(;.*)?$", line)
        if m and NAME.match(m.group(1)):
            k, up, w, nt = NAME.match(m.group(1)).groups()
            cur = out.setdefault((int(k), up == "1", int(w), nt == "1"), [])
            continue
        if cur is not None:
            cur.append(line)
            if line.lstrip().startswith("; ScratchSize:"):      # the last of the resource comments that follow the kernel
                cur = None
    return out


def is_full_wait(ins):
    return ins.startswith("s_waitcnt") and "vmcnt(0)" in ins


def measure(lines):
    """counts of one kernel; pairs: (load, source location of the load or None)"""
    loads = waits = 0
    pairs = []
    prev, loc, prev_loc = None, None, None
    res = {}
    for line in lines:
        t = line.strip()
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", t)
        if m:
            loc = (int(m.group(1)), int(m.group(2)))
            continue
        m = re.match(r";\s*(NumVgprs|ScratchSize|NumAgprs|Occupancy):\s*(\d+)", t)
        if m:
            res[m.group(1)] = int(m.group(2))
            continue
        if not t or t[0] in ";." or t.endswith(":"):      # comments, directives, labels
            continue
        ins = t.split(";")[0].strip()
        if ins.startswith("global_load") or ins.startswith("flat_load") or ins.startswith("buffer_load"):
            loads += 1
        if is_full_wait(ins):
            waits += 1
            if prev is not None and (prev.startswith("global_load") or prev.startswith("flat_load") or prev.startswith("buffer_load")):
                pairs.append((prev, prev_loc))
        prev, prev_loc = ins, loc
    return dict(loads=loads, waits=waits, pairs=pairs, vgprs=res.get("NumVgprs", -1), agprs=res.get("NumAgprs", 0), scratch=res.get("ScratchSize", -1))


def report(asm):
    rows = []
    for key, lines in sorted(tier_kernels(asm).items(), key=lambda kv: (kv[0][2], kv[0][3], kv[0][0], not kv[0][1])):
        rows.append((key, measure(lines)))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", action="store_true", help="list every load + full wait pair with the source line of the load")
    ap.add_argument("--asm", help="write the assembly here")
    a = ap.parse_args()
    asm = assembly(["-g1"] if a.pairs else [])
    if a.asm:
        open(a.asm, "w").write(asm)
    rows = report(asm)
    if not rows:
        sys.exit("no k_nd_tier instantiation found in the assembly")
    print("| kernel | global loads | full waits | full wait directly after a load | VGPRs | scratch |")
    print("|---|---|---|---|---|---|")
    for (k, up, w, nt), m in rows:
        name = f"`k_nd_tier<{k},{'true' if up else 'false'},{w},{'true' if nt else 'false'}>` ({'up' if up else 'down'})"
        print(f"| {name} | {m['loads']} | {m['waits']} | {len(m['pairs'])} | {m['vgprs']} | {m['scratch']} |")
    if a.pairs:
        # .file <n> ["<directory>"] "<name>" -> the source line a .loc points to
        files = {int(m.group(1)): m.group(2) for m in re.finditer(r'^\s*\.file\s+(\d+)\s+(?:"[^"]*"\s+)?"([^"]+)"', asm, re.M)}
        text_of = {}
        for (k, up, w, nt), m in rows:
            print(f"\nk_nd_tier<{k},{'true' if up else 'false'},{w},{'true' if nt else 'false'}>:")
            for ins, loc in m["pairs"]:
                name = os.path.basename(files.get(loc[0], "?")) if loc else "?"
                path = os.path.join(CSRC, name)
                if name not in text_of:
                    text_of[name] = open(path).read().splitlines() if os.path.isfile(path) else []
                src = text_of[name]
                text = src[loc[1] - 1].strip() if loc and 0 < loc[1] <= len(src) else "?"
                print(f"    {ins.split()[0]:22s} {name}:{loc[1] if loc else '?'}: {text[:110]}")
    bad = [key for key, m in rows if m["scratch"] != 0 or m["vgprs"] > 128]
    if bad:
        sys.exit(f"over the register budget (128 VGPRs, scratch 0): {bad}")


if __name__ == "__main__":
    main()
