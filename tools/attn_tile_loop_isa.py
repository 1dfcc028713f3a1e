"""Diagnostic (build container, no GPU): what the compiler makes of the tile loop of attn_fwd3_kernel (csrc/attention3.hip).
Compiles the file to gfx950 assembly (or reads a given .s), and for every instantiation of the kernel prints, per loop that
holds MFMAs, the phases of 16 MFMAs in program order: basic blocks and branches between the first and the last MFMA of the
phase, the opcode counts of the window, and the vector instructions of each MFMA gap.  Also: every run of >= 4 consecutive
v_add_f32, compares / selects per loop, code bytes, and the register / spill / LDS / occupancy remarks.
usage: python tools/attn_tile_loop_isa.py [--asm FILE.s --remarks FILE.txt] [--detail 'I4BF16Li8ELi0E'] [-DFLAG ...]"""
import collections
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "memory-augmented-vlm_amd", "csrc", "attention3.hip")
KERNEL = "attn_fwd3_kernel"


def compile_asm(flags):
    import shutil
    import tempfile
    out = os.path.join(tempfile.mkdtemp(prefix="attn3_isa_"), "attention3.s")
    cmd = [shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
           "-Rpass-analysis=kernel-resource-usage", "-o", out, SRC] + flags
    r = subprocess.run(cmd, check=True, stderr=subprocess.PIPE, text=True)
    return open(out).read(), r.stderr


def functions(s):
    for m in re.finditer(r"^(_Z\S*" + KERNEL + r"\S*):[^\n]*\n(.*?)\.Lfunc_end\d+:", s, re.S | re.M):
        yield m.group(1), m.group(2)


def blocks(body):
    """[(label, loop header or None, depth, [instruction lines])] in text order"""
    out, cur = [], None
    lines = body.split("\n")
    for idx, line in enumerate(lines):
        t = line.strip()
        m = re.match(r"(\.LBB\d+_\d+):|; %bb\.(\d+):", t)
        if m:
            label = m.group(1) or "bb." + m.group(2)
            ctx = t + " " + (lines[idx + 1].strip() if idx + 1 < len(lines) and lines[idx + 1].strip().startswith(";") and
                             "%bb" not in lines[idx + 1] else "")
            d = re.findall(r"Depth=(\d+)", ctx)
            depth = max(map(int, d)) if d else 0
            h = re.search(r"in Loop: Header=(BB\d+_\d+)", ctx)
            header = h.group(1) if h else (label.lstrip(".L") if "Loop Header" in ctx else None)
            cur = (label, header, depth, [])
            out.append(cur)
            continue
        if not t or t.startswith(";") or t.startswith("."):
            continue
        if cur is None:
            cur = ("entry", None, 0, [])
            out.append(cur)
        cur[3].append(t.split(";")[0].strip())
    return out


def op(t):
    return t.split()[0]


def short(o):
    return re.sub(r"_e(32|64)$", "", o)


def analyse(name, body, detail):
    bl = blocks(body)
    loops = collections.OrderedDict()
    for b in bl:
        if b[2] >= 2 and b[1]:
            loops.setdefault(b[1], []).append(b)
    res = []
    for header, lb in loops.items():
        seq = []                                        # (block label, instruction)
        for b in lb:
            seq += [(b[0], t) for t in b[3]]
        mf = [i for i, (_, t) in enumerate(seq) if op(t).startswith("v_mfma")]
        if not mf:
            continue
        cmpsel = collections.Counter(short(op(t)).rsplit("_", 1)[0] if op(t).startswith("v_cmp") else short(op(t))
                                     for _, t in seq if op(t).startswith(("v_cmp", "v_cndmask", "v_readlane", "v_writelane")))
        res.append(f"  loop {header}: {len(lb)} blocks, {len(seq)} instructions, {len(mf)} MFMAs; compares/selects/lane moves: "
                   + (", ".join(f"{k} {v}" for k, v in sorted(cmpsel.items())) or "none"))
        for p in range(0, len(mf), 16):
            ph = mf[p:p + 16]
            win = seq[ph[0]:ph[-1] + 1]
            nblk = len(set(l for l, _ in win))
            nbr = sum(1 for _, t in win if op(t).startswith(("s_cbranch", "s_branch")))
            cnt = collections.Counter(short(op(t)) for _, t in win)
            kind = "A" if cnt.get("v_exp_f32", 0) else "B"
            gaps = []
            for a, b in zip(ph[:-1], ph[1:]):
                g = [short(op(t)) for _, t in seq[a + 1:b] if op(t).startswith("v_") or op(t) == "s_nop"]
                gaps.append(g)
            gsum = collections.Counter(tuple(sorted(collections.Counter(g).items())) for g in gaps)
            res.append(f"    phase {p // 16} [{kind}]: {len(ph)} MFMAs in {nblk} basic block(s), {nbr} branches inside; "
                       + " ".join(f"{k}={cnt[k]}" for k in ("v_fma_f32", "v_exp_f32", "v_add_f32", "v_max3_f32", "v_mov_b32",
                                                             "s_nop", "v_cvt_pk_bf16_f32", "v_cvt_pkrtz_f16_f32", "v_perm_b32",
                                                             "ds_read_b128", "ds_read_b64_tr_b16", "buffer_load_dwordx4",
                                                             "s_waitcnt") if cnt.get(k)))
            if detail:
                for g, n in gsum.most_common():
                    res.append(f"        {n:2d} gap(s): " + (", ".join(f"{k} x{v}" for k, v in g) or "(no VALU)"))
    # runs of consecutive v_add_f32 anywhere in the kernel
    runs = []
    for b in bl:
        n = 0
        for t in b[3] + ["end"]:
            if short(op(t)) == "v_add_f32":
                n += 1
            else:
                if n >= 4:
                    runs.append((b[0], b[2], n))
                n = 0
    res.append("  runs of >= 4 consecutive v_add_f32: " +
               (", ".join(f"{n} in {l} (depth {d})" for l, d, n in runs) or "none"))
    nb = sum(1 for b in bl for t in b[3] if op(t).startswith("s_cbranch"))
    near = 0
    flat = [t for b in bl for t in b[3]]
    for i, t in enumerate(flat):
        if op(t).startswith("s_cbranch") and any(op(x).startswith("v_mfma") for x in flat[max(0, i - 2):i + 3]):
            near += 1
    res.append(f"  s_cbranch in the kernel: {nb}, of them within two instructions of an MFMA: {near}")
    return res


def main():
    args = sys.argv[1:]
    asm = remarks = detail = None
    flags = []
    while args:
        a = args.pop(0)
        if a == "--asm": asm = args.pop(0)
        elif a == "--remarks": remarks = args.pop(0)
        elif a == "--detail": detail = args.pop(0)
        else: flags.append(a)
    if asm:
        s, rem = open(asm).read(), (open(remarks).read() if remarks else "")
    else:
        s, rem = compile_asm(flags)
    usage = {}
    for m in re.finditer(r"Function Name: (\S+) \[.*?(?=Function Name:|\Z)", rem, re.S):
        f = dict(re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", m.group(0)))
        usage[m.group(1)] = f
    total = 0
    for name, body in functions(s):
        code = re.search(re.escape(name) + r":.*?; codeLenInByte = (\d+)", s, re.S)
        nbytes = int(code.group(1)) if code else -1
        total += nbytes
        print("==", name)
        u = usage.get(name, {})
        print(f"  code bytes {nbytes}; " + "; ".join(f"{k} {v}" for k, v in u.items()))
        for line in analyse(name, body, detail is not None and detail in name):
            print(line)
    print(f"== code bytes of all {KERNEL} instantiations: {total}")


if __name__ == "__main__":
    main()
