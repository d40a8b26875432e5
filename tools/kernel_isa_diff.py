#!/usr/bin/env python
"""kernel_isa_diff.py libA.so libB.so [regex] -- per kernel of two builds of libgrlx.so: is the gfx950 instruction stream the
same, and what do the registers, the scratch and the LDS come to (A -> B where they differ).  CPU only: the code objects
are taken out of the libraries and disassembled with the ROCm LLVM tools the build uses.  The assembly-filter reports
(libgrlx.so.asmfix) of both builds are printed first."""
import glob, os, re, shutil, subprocess, sys, tempfile

LLVM = next(d for d in ("/opt/rocm/lib/llvm/bin", "/opt/rocm/llvm/bin") if os.path.exists(os.path.join(d, "llvm-objdump")))
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def tool(name, *args, cwd=None):
    return subprocess.run([os.path.join(LLVM, name)] + list(args), cwd=cwd, capture_output=True, text=True, check=True).stdout


def kernels(lib):
    """{kernel symbol: (normalised instruction list, {metadata field: value})} over every gfx950 code object in `lib`"""
    out = {}
    with tempfile.TemporaryDirectory(prefix="isa_diff_") as tmp:
        shutil.copy(lib, os.path.join(tmp, "lib.so"))
        tool("llvm-objdump", "--offloading", "lib.so", cwd=tmp)          # writes lib.so.<n>.<target> next to the input
        for co in sorted(glob.glob(os.path.join(tmp, "lib.so.*gfx950"))):
            meta, cur, kcol = {}, None, 0
            for ln in tool("llvm-readelf", "--notes", co).split("\n"):
                m = re.match(r"\s*(?:- )?(\.\w+):\s+(.*)$", ln)
                if not m:
                    continue
                col = ln.index(".")
                if ln.lstrip().startswith("- .agpr_count"):
                    cur, kcol = {}, col                                   # first key of a kernel's entry (keys are sorted)
                if cur is None or col != kcol:
                    continue                                              # (an argument's keys sit deeper)
                if m.group(1) in FIELDS:
                    cur[m.group(1)] = int(m.group(2))
                if m.group(1) == ".name":
                    meta[m.group(2).strip("'\"")] = cur
            name, body, getpc = None, {}, 0
            for ln in tool("llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co).split("\n"):
                m = re.match(r"^[0-9a-f]* ?<([^>]+)>:$", ln)
                if m:
                    name = m.group(1)
                    body[name] = []
                    continue
                ins = ln.split("//")[0].strip()
                if name is None or not ins or ins == "...":               # "...": objdump's elision of the zero padding up to the next symbol's alignment
                    continue
                # pc-relative addresses of other symbols move with every other kernel's size: not part of this kernel's code
                getpc = 3 if ins.startswith("s_getpc_b64") else getpc - 1
                if getpc > 0 and re.match(r"s_addc?_u32 ", ins):
                    ins = re.sub(r"(0x[0-9a-f]+|-?\d+)$", "<pcrel>", ins)
                body[name].append(ins)
            kd = set(re.findall(r"(\S+)\.kd\b", tool("llvm-readelf", "--symbols", "--wide", co)))      # kernel descriptors: one per kernel
            if kd != set(meta) or any(k not in body for k in meta):
                print(f"WARNING {os.path.basename(co)}: {len(kd)} kernel descriptors, {len(meta)} metadata entries, "
                      f"{sum(k in body for k in meta)} of them disassembled: the table below is incomplete")
            for k, v in meta.items():
                out[k] = (body.get(k, []), v)
    return out


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    rx = re.compile(sys.argv[3]) if len(sys.argv) > 3 else None
    for lib in sys.argv[1:3]:
        fix = lib + ".asmfix"
        print(lib + ": " + (open(fix).read().strip().replace("\n", "; ") if os.path.exists(fix) else "no .asmfix report"))
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    names = sorted(k for k in set(a) | set(b) if not rx or rx.search(k))        # mangled symbols; the regex applies to them
    print("| kernel | code | vgpr | agpr | sgpr | scratch B | LDS B |\n|---|---|---|---|---|---|---|")
    n_diff = 0
    for k in names:
        if k not in a or k not in b:
            one = a[k] if k in a else b[k]                                   # a kernel of one build only: its own figures
            print(f"| `{k}` | only in {'A' if k in a else 'B'} ({len(one[0])} instructions) | " + " | ".join(str(one[1].get(f)) for f in FIELDS) + " |")
            n_diff += 1
            continue
        same = a[k][0] == b[k][0]
        n_diff += 0 if same else 1
        cols = [str(a[k][1].get(f)) if a[k][1].get(f) == b[k][1].get(f) else f"{a[k][1].get(f)} -> {b[k][1].get(f)}" for f in FIELDS]
        code = "identical" if same else f"differs ({len(a[k][0])} -> {len(b[k][0])} instructions)"
        print(f"| `{k}` | {code} | " + " | ".join(cols) + " |")
    print(f"{len(names)} kernels, {n_diff} differ")


if __name__ == "__main__":
    main()
