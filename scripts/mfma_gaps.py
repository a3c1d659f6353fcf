#!/usr/bin/env python3
"""What stands between the MFMAs of a kernel whose wave is alone on its SIMD (csrc/hg_bt_wino_f32.h: nothing vector hides there).

    python scripts/mfma_gaps.py LISTING.s|libdf3d_hip.so|CODE_OBJECT SUBSTRING [SUBSTRING ...] [--json]

LISTING.s is hipcc's assembly (-S --offload-device-only); a shared library or a gfx950 code object is disassembled with llvm-objdump.
For every kernel whose demangled or mangled name contains one of the substrings, inside the kernel's outermost loop (the persistent
kernels' tile loop; the whole body if there is none):

  exposed   triples `ds_read*`, `s_waitcnt lgkmcnt(0)`, `v_mfma*` on consecutive instructions: an LDS fragment read whose whole latency the
            wave sits out in front of the MFMA that consumes it (a pipelined read is followed by other work, or waited for with a count > 0);
  far_adds  `v_add_u32` with a literal >= 0x10000 (65 536): LDS addresses past the 16-bit immediate offset of the base they are formed from, each a
            VGPR that lives until its read;
  gaps      per inner loop (phase 2's chunk loop): the runs of instructions between two MFMAs that hold vector-ALU instructions, as
            (number of runs, instructions in them), with the runs of CLUMP or more -- the intended transform clumps -- counted apart; and the
            v_accvgpr_* instructions among them.
"""
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

CLUMP = 32
LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")


def tool(name):
    p = os.path.join(LLVM, name)
    return p if os.path.exists(p) else shutil.which(name)


def demangle(names):
    cf = tool("llvm-cxxfilt") or shutil.which("c++filt")
    if not cf or not names:
        return list(names)
    out = subprocess.run([cf], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return [d or n for n, d in zip(names, out)]


def from_listing(path, subs):
    """-> {mangled name: [(label or None, opcode, operands)]}"""
    kernels, cur = {}, None
    for line in open(path, errors="replace"):
        t = line.split(";")[0].rstrip()
        if not t.strip():
            continue
        if not t[0].isspace() and t.endswith(":"):
            name = t[:-1]
            if name.startswith("_Z"):
                cur = kernels.setdefault(name, [])
            elif cur is not None:
                cur.append((name, None, ""))
            continue
        s = t.strip()
        if s.startswith(".") or cur is None:
            if s.startswith(".end_amdhsa_kernel") or s.startswith(".section"):
                cur = None
            continue
        parts = s.split(None, 1)
        cur.append((None, parts[0], parts[1] if len(parts) > 1 else ""))
        if parts[0] == "s_endpgm":
            cur = None
    names = list(kernels)
    dem = dict(zip(names, demangle(names)))
    return {dem[n]: normalise_labels(v) for n, v in kernels.items() if any(s in n or s in dem[n] for s in subs)}


def normalise_labels(ins):
    """labels -> instruction indices; branches carry the index of their target"""
    at, out = {}, []
    for lab, op, args in ins:
        if op is None:
            at[lab] = len(out)
        else:
            out.append([op, args, None])
    for rec in out:
        if rec[0].startswith(("s_cbranch", "s_branch")) and rec[1].strip() in at:
            rec[2] = at[rec[1].strip()]
    return out


def from_binary(path, subs):
    od = tool("llvm-objdump")
    if not od:
        sys.exit("llvm-objdump not found")
    tmp = tempfile.mkdtemp(prefix="mfma_gaps_")
    try:
        objs = [path]
        if open(path, "rb").read(20)[18:20] != b"\xe0\x00":   # e_machine of an x86 host library is not EM_AMDGPU (224): unbundle it
            lib = os.path.join(tmp, "lib.so")
            shutil.copy(path, lib)
            subprocess.run([od, "--offloading", lib], cwd=tmp, capture_output=True, text=True)
            objs = sorted(glob.glob(os.path.join(tmp, "*gfx950*")))
        found = {}
        for obj in objs:
            syms = subprocess.run([od, "-t", obj], capture_output=True, text=True).stdout.split("\n")
            names = sorted({l.split()[-1] for l in syms if " F " in l and l.split()[-1].startswith("_Z")})
            dem = dict(zip(names, demangle(names)))
            want = [n for n in names if any(s in n or s in dem[n] for s in subs)]
            if not want:
                continue
            txt = subprocess.run([od, "-d", "--no-show-raw-insn", "--disassemble-symbols=" + ",".join(want), obj], capture_output=True, text=True).stdout
            cur, addr_of = None, {}
            for line in txt.split("\n"):
                m = re.match(r"^([0-9a-f]+) <(\S+)>:", line)
                if m:
                    cur = found.setdefault(dem.get(m.group(2), m.group(2)), [])
                    addr_of[id(cur)] = {}
                    continue
                m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", line)
                if m and cur is not None:
                    addr_of[id(cur)][int(m.group(3), 16)] = len(cur)
                    cur.append([m.group(1), m.group(2), None])
            for ins in found.values():
                amap = addr_of.get(id(ins), {})
                for k, rec in enumerate(ins):   # a branch's operand is a signed dword offset from the next instruction
                    if rec[0].startswith(("s_cbranch", "s_branch")):
                        m = re.match(r"^(-?\d+)", rec[1].strip())
                        if m:
                            here = [a for a, i in amap.items() if i == k][0]
                            off = int(m.group(1))
                            off = off - 65536 if off >= 32768 else off
                            rec[2] = amap.get(here + 4 + 4 * off)
        return found
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def is_mfma(op):
    return op.startswith(("v_mfma", "v_smfmac"))


def is_valu(op):
    return op.startswith("v_") and not is_mfma(op)


def analyse(ins):
    loops = sorted({(rec[2], k) for k, rec in enumerate(ins) if rec[2] is not None and rec[2] <= k})
    outer = max(loops, key=lambda r: r[1] - r[0]) if loops else (0, len(ins) - 1)
    lo, hi = outer
    exposed = sum(1 for k in range(lo, hi - 1)
                  if ins[k][0].startswith("ds_read") and ins[k + 1][0] == "s_waitcnt" and re.search(r"lgkmcnt\(0\)", ins[k + 1][1]) and is_mfma(ins[k + 2][0]))
    far = []
    for k in range(lo, hi + 1):
        if ins[k][0].startswith("v_add_u32"):
            for a in ins[k][1].split(","):
                a = a.strip()
                if re.fullmatch(r"0x[0-9a-fA-F]+|\d+", a) and 0x10000 <= int(a, 0) < 0x80000000:   # (not a negative constant)
                    far.append(a)
    inner = []
    for l0, l1 in loops:
        if not (lo <= l0 and l1 <= hi) or (l0, l1) == outer:
            continue   # the loops inside the outermost one
        n_mfma = sum(1 for k in range(l0, l1 + 1) if is_mfma(ins[k][0]))
        if n_mfma < 8 or n_mfma == sum(1 for k in range(lo, hi + 1) if is_mfma(ins[k][0])):
            continue   # (a second back edge of the tile loop itself)
        runs, run, seen = [], None, False
        for k in range(l0, l1 + 1):
            op = ins[k][0]
            if is_mfma(op):
                if seen and run and run[0]:
                    runs.append(run)
                run, seen = [0, 0], True
            elif run is not None and is_valu(op):
                run[0] += 1
                run[1] += op.startswith("v_accvgpr")
        clumps = [r for r in runs if r[0] >= CLUMP]
        small = [r for r in runs if r[0] < CLUMP]
        inner.append({"mfma": n_mfma, "clumps": [r[0] for r in clumps], "gaps": len(small), "gap_valu": sum(r[0] for r in small),
                      "accvgpr": sum(r[1] for r in runs)})
    return {"instructions": len(ins), "tile_loop": hi - lo + 1 if loops else 0, "mfma": sum(1 for r in ins if is_mfma(r[0])), "exposed": exposed,
            "far_adds": len(far), "far_literals": sorted(set(far)), "inner_loops": inner}


def run(path, subs):
    kernels = from_listing(path, subs) if path.endswith((".s", ".S", ".asm")) else from_binary(path, subs)
    return {name: analyse(ins) for name, ins in sorted(kernels.items())}


def main():
    args = [a for a in sys.argv[1:] if a != "--json"]
    if len(args) < 2:
        sys.exit(__doc__)
    res = run(args[0], args[1:])
    if not res:
        sys.exit(f"no kernel matching {args[1:]}")
    if "--json" in sys.argv:
        print(json.dumps(res, indent=1))
        return
    for name, r in res.items():
        print(f"{name[:96]}\n    {r['mfma']} MFMAs; exposed ds_read/lgkmcnt(0)/mfma triples {r['exposed']}; far address adds {r['far_adds']} {r['far_literals'][:4]}")
        for l in r["inner_loops"]:
            print(f"    loop of {l['mfma']} MFMAs: clumps {l['clumps']}, {l['gaps']} other gaps with {l['gap_valu']} VALU ops; v_accvgpr_* between MFMAs {l['accvgpr']}")


if __name__ == "__main__":
    main()
