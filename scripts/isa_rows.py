"""Static VALU instructions of one gca_alex_march.hip kernel instance by source line (ISA analysis; no GPU).
Compiles the R = 6 instances only (-DGCA_MARCH_ANALYSIS_R6) to device assembly with line info and counts, for the
instance named by its template flags, the VALU instructions attributed to each source line, largest first.
Then the row loop (the kernel's largest loop by the compiler's block annotations; its body is two rows): VALU / SALU /
LDS instructions per row on the main path, and the v_writelane / v_readlane (SGPR spills to VGPR lanes) inside the loop. The main path is
the walk from the loop's head to its backward branch that, at every forward branch, takes the longer side (a row that
needs the heat and direction passes and draws) except at the branches of RARE below (the dousing windows, the second
Philox block), where it takes the shorter.
Usage: python scripts/isa_rows.py [OBS GROW NSEG FLATM] (default 0 0 1 2: the headline step, flat terrain + uniform
layers); --src PATH analyses another copy of the source, extra -D... arguments go to the compiler."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gym-cellular-automata_amd", "csrc", "gca_alex_march.hip")
# source text of the conditions the main path does not take: a forward branch is "rare" when one of its two successor
# blocks holds instructions of the lines inside such an `if`'s braces (and the other does not)
RARE = ("if (dous_any)", "if (__ballot((burn & (burn - 1u)) != 0u) != 0ull)")
RARE_ELSE = ("if (!p.burnout_eq1)",)  # the same for the `else` of these (the classic burn-out rule)


def rare_lines(src_lines):
    out = set()
    def block_end(i):  # the line whose brace closes the block opened on line i
        depth, j = 0, i
        while True:
            depth += src_lines[j].count("{") - src_lines[j].count("}")
            if depth <= 0 and j > i:
                return j
            j += 1

    for i, l in enumerate(src_lines):
        if any(r in l for r in RARE):
            out.update(range(i + 2, block_end(i) + 2))
        if any(r in l for r in RARE_ELSE):
            j, depth = i + 1, 1
            while not (depth == 1 and src_lines[j].strip().startswith("} else")):
                depth += src_lines[j].count("{") - src_lines[j].count("}")
                j += 1
            out.update(range(j + 2, block_end(i) + 1))  # the lines between "} else {" and the closing brace
    return out


def kernel_lines(src, name, flags=()):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "gca_march_r6.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-g", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-munsafe-fp-atomics", "-DGCA_MARCH_ANALYSIS_R6", *flags, "--cuda-device-only", "-S", src,
                        "-o", out], check=True, stderr=subprocess.DEVNULL)
        L = open(out).read().split("\n")
    s = next(i for i, l in enumerate(L) if l.startswith("_Z") and name in l.split(":")[0])
    e = next(i for i in range(s, len(L)) if L[i].startswith(".Lfunc_end"))  # (not the first s_endpgm: early returns)
    files = {}
    for l in L:
        m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
        if m:
            files[m.group(1)] = (m.group(3) or m.group(2)).split("/")[-1]
    return L[s:e + 1], files


def row_loop(K, files, src_lines, src_name):
    """Basic blocks of the kernel's largest loop (the compiler's own `Header=` block annotations) and the main-path
    walk through them: from the header until a branch returns to it or leaves the loop."""
    # blocks: a new block at every label / fall-through block comment and after every branch
    blocks, loc = [], None

    def new_block(label=None, comment=""):
        b = {"label": label, "n": collections.Counter(), "rare": False, "branch": None, "loop": None, "lines": set()}
        m = re.search(r"Header=(BB\d+_\d+)", comment)
        if m:
            b["loop"] = m.group(1)
        elif "Loop Header" in comment and label:
            b["loop"] = label[2:]  # .LBBn_m heads the loop BBn_m
        blocks.append(b)
        return b

    cur = new_block()
    for l in K:
        t = l.strip()
        m = re.match(r"(\.LBB\d+_\d+):(.*)", t) or re.match(r"; (%bb\.\d+):(.*)", t)
        if m:
            if cur["n"] or cur["branch"] or cur["label"]:
                cur = new_block()
            cur["label"] = m.group(1)
            mm = re.search(r"Header=(BB\d+_\d+)", m.group(2))
            cur["loop"] = mm.group(1) if mm else (m.group(1)[2:] if "Loop Header" in m.group(2) else None)
            continue
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", t)
        if m:
            loc = (files.get(m.group(1), m.group(1)), int(m.group(2)))
            continue
        if not t or t.startswith((";", ".")):
            continue
        op = t.split()[0]
        kind = ("spill" if op.startswith(("v_writelane", "v_readlane")) else "valu" if op.startswith("v_") else
                "salu" if op.startswith("s_") and not op.startswith(("s_waitcnt", "s_nop", "s_cbranch", "s_branch")) else
                "lds" if op.startswith("ds_") else "vmem" if op.startswith(("global_", "buffer_", "flat_")) else "other")
        cur["n"][kind] += 1
        if loc and loc[0] == src_name:
            cur["lines"].add(loc[1])
        m = re.match(r"s_(cbranch_\w+|branch)\s+(\.LBB\d+_\d+)", t)
        if m:
            cur["branch"] = (m.group(1) != "branch", m.group(2))
            nb = new_block()
            nb["loop"] = cur["loop"]  # the code behind a branch stays in its block's loop until a label says otherwise
            cur = nb
    size = collections.Counter()
    for b in blocks:
        if b["loop"]:
            size[b["loop"]] += sum(b["n"].values())
    if not size:
        return None
    head = size.most_common(1)[0][0]
    inloop = [k for k, b in enumerate(blocks) if b["loop"] == head]
    tot = collections.Counter()
    for k in inloop:
        tot.update(blocks[k]["n"])
    by_label = {b["label"]: k for k, b in enumerate(blocks) if b["label"]}
    hk = by_label[".L" + head]
    memo = {}
    rare = rare_lines(src_lines)

    def walk(k, first=False):  # (valu, salu, lds) of the main path from block k to the loop's end
        if k >= len(blocks) or blocks[k]["loop"] != head or (k == hk and not first):
            return (0, 0, 0)
        if k in memo:
            return memo[k]
        memo[k] = (0, 0, 0)  # (a cycle that avoids the header: none in this kernel; ends the walk)
        b = blocks[k]
        own = (b["n"]["valu"] + b["n"]["spill"], b["n"]["salu"], b["n"]["lds"])  # the lane moves issue on the VALU too
        br = b["branch"]
        nxt = []
        if br is None or br[0]:
            nxt.append(k + 1)  # falls through
        if br is not None and br[1] in by_label:
            nxt.append(by_label[br[1]])
        rest = [walk(n) for n in nxt] or [(0, 0, 0)]
        in_rare = [n < len(blocks) and bool(blocks[n]["lines"] & rare) for n in nxt]
        b["rare"] = len(nxt) == 2 and in_rare[0] != in_rare[1]
        pick = rest[in_rare.index(False)] if b["rare"] else max(rest)
        memo[k] = tuple(a + c for a, c in zip(own, pick))
        return memo[k]

    sys.setrecursionlimit(10000)
    return {"total": tot, "main": walk(hk, True), "blocks": len(inloop),
            "rare_found": sum(1 for k in inloop if blocks[k]["rare"])}


def main(obs=0, grow=0, nseg=1, flat=1, top=40, src=SRC, flags=()):
    name = f"alex_march_kernelILi6ELb{obs}ELb{grow}ELi{nseg}ELi{flat}E"
    K, files = kernel_lines(src, name, flags)
    cur, cnt, ops, tot = None, collections.Counter(), collections.Counter(), 0
    for l in K:
        t = l.strip()
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", t)
        if m:
            cur = (files.get(m.group(1), m.group(1)), int(m.group(2)))
            continue
        if t.startswith("v_"):
            cnt[cur] += 1
            ops[t.split()[0]] += 1
            tot += 1
    src_lines = open(src).read().split("\n")
    print(f"{name}: {tot} VALU (static, whole kernel)")
    for (f, ln), v in cnt.most_common(top):
        text = src_lines[ln - 1].strip()[:110] if f == os.path.basename(src) and ln else ""
        print(f"{v:5d}  {f}:{ln}  {text}")
    print(" ".join(f"{k}:{v}" for k, v in ops.most_common(25)))
    loop = row_loop(K, files, src_lines, os.path.basename(src))
    if loop is None:
        print("row loop: no backward branch found")
        return
    v, s, d = loop["main"]
    t = loop["total"]
    print(f"row loop (2 rows per pass, {loop['blocks']} blocks, {loop['rare_found']} rare branches recognised): "
          f"main path per row VALU {v / 2:.1f} SALU {s / 2:.1f} LDS {d / 2:.1f}; "
          f"all paths VALU {t['valu']} SALU {t['salu']} LDS {t['lds']} VMEM {t['vmem']}; "
          f"v_writelane / v_readlane in the loop: {t['spill']}")


if __name__ == "__main__":
    argv = sys.argv[1:]
    src = SRC
    if "--src" in argv:
        i = argv.index("--src")
        src = argv[i + 1]
        del argv[i:i + 2]
    flags = tuple(x for x in argv if x.startswith("-D"))
    argv = [x for x in argv if not x.startswith("-D")]
    a = [int(x) for x in argv[:4]] if len(argv) >= 4 else [0, 0, 1, 2]
    main(*a, src=src, flags=flags)
