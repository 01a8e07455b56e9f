#!/usr/bin/env python3
"""Does the direct-to-LDS ring of gemm_glds_kernel.h / wgrad3x3.hip exist in the generated code?

The kernels keep k-tiles in flight under the MFMAs of the current one: LDS-DMA loads (buffer_load ... lds) retired by a COUNTED
`s_waitcnt vmcnt(G)` / `vmcnt(2G)` ahead of a raw `s_barrier`.  That only works if nothing else drains the load queue.  hipcc treats
the transpose-read builtin (ds_read_b64_tr_b16) as possibly aliasing the pending LDS-DMA writes and puts an `s_waitcnt vmcnt(0)`
in front of every group of such reads: every tile in flight is waited for at each k-step and the counted waits are dead code.

This tool compiles the shipped units to assembly with the Makefile's flags (no GPU needed) and reports, per kernel function,
  drains   `s_waitcnt` with vmcnt(0) directly followed by a ds_read* instruction          (must be 0)
  counted  the distinct counted waits `vmcnt(N)`, N > 0, of the function                   (must contain G and 2G)
Exit status 1 when a function misses either property.

    python tools/check_lds_ring_waits.py [--keep DIR] [-v]
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "show-attend-and-tell-pytorch-lightning_amd", "csrc")

# template arguments of gemm_glds_kernel<BM, BN, WR, WC, AM, BMo, TC, APF> as the Itanium mangling spells them
_GLDS = re.compile(r"^_ZN3sat16gemm_glds_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E(\w+?)Lb([01])EEEvNS_5BArgsE$")
_TYPES = {"DF16b": "bf16", "f": "float"}
A_KMAJOR = 1          # gemm_bf16_common.h: A_ROW 0, A_KMAJOR 1, A_CONV_FWD 2, A_CONV_DGRAD 3; B_ROW 0, B_KMAJOR 1, B_CONV_WGRAD 2, B_CONV_DGRAD_W 3
_WAIT = re.compile(r"^s_waitcnt\b(.*)$")
_VMCNT = re.compile(r"vmcnt\((\d+)\)")


def hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


def makefile_flags():
    """arch, language level and the unroll threshold of the tile units, read from csrc/Makefile"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = ["--offload-arch=" + arch] + re.findall(r"(?<=\s)(-O\d|-std=\S+)", re.search(r"^CXXFLAGS\s*=(.*)$", text, re.M).group(1))
    tile = re.search(r"^build/gemm_glds_t%\.o:\s*CXXFLAGS\s*\+=\s*((?:-mllvm\s+\S+\s*)+)", text, re.M)
    return flags, (tile.group(1).split() if tile else [])


def units():
    text = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", text, re.M).group(1).split()
    return [s for s in srcs if re.match(r"gemm_glds_t\w+\.hip$", s) or s == "wgrad3x3.hip"]


def compile_to_asm(unit, outdir):
    flags, tile_flags = makefile_flags()
    out = os.path.join(outdir, unit.replace(".hip", ".s"))
    cmd = [hipcc()] + flags + ["-I../../include"] + (tile_flags if unit.startswith("gemm_glds_t") else []) + ["--cuda-device-only", "-S", unit, "-o", out]
    subprocess.run(cmd, cwd=CSRC, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return out


def functions(path):
    """{kernel symbol: [instruction lines]} of the .amdhsa kernels of an assembly file"""
    funcs, name = {}, None
    for raw in open(path):
        line = raw.split(";")[0].strip()
        if not line:
            continue
        m = re.match(r"^(\w+):$", line)
        if m and raw[0] not in " \t" and not line.startswith(".L"):
            name = m.group(1)
            funcs[name] = []
            continue
        if line.startswith(".end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            name = None
        if name is None or line.startswith(".") or line.endswith(":"):
            continue
        funcs[name].append(line)
    return {k: v for k, v in funcs.items() if any(i.startswith("s_endpgm") for i in v)}


def analyse(insts):
    drains, counted = 0, set()
    for cur, nxt in zip(insts, insts[1:] + [""]):
        m = _WAIT.match(cur)
        if not m:
            continue
        for n in _VMCNT.findall(m.group(1)):
            if int(n) > 0:
                counted.add(int(n))
            elif nxt.startswith("ds_read"):
                drains += 1
    return drains, counted


def describe(symbol):
    """(label, G or None, transposing): G = LDS-DMA instructions per wave and k-tile, whose multiples the counted waits name"""
    m = _GLDS.match(symbol)
    if m:
        bm, bn, wr, wc, am, bmo = (int(x) for x in m.groups()[:6])
        tc = _TYPES.get(m.group(7), m.group(7))
        g = bm // (8 * wr * wc) + bn // (8 * wr * wc)
        return "gemm_glds<%dx%d,(%d,%d),%s%s>" % (bm, bn, am, bmo, tc, ",apf" if m.group(8) == "1" else ""), g, am == A_KMAJOR or bmo != 0
    if "wgrad3x3_kernel" in symbol:
        return "wgrad3x3", None, True
    return symbol, None, False


def check_unit(asm_path):
    """[(label, drains, counted waits, missing counted waits)] per kernel of the file"""
    rows = []
    for symbol, insts in sorted(functions(asm_path).items()):
        label, g, _ = describe(symbol)
        if label == symbol:
            continue          # split-K reduce and other helpers: no ring
        drains, counted = analyse(insts)
        want = {g, 2 * g} if g else {2, 3, 4}          # wgrad3x3: a wave issues 2, 3 or 4 pieces per k-tile
        rows.append((label, drains, sorted(counted), sorted(want - counted)))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--keep", metavar="DIR", help="write the assembly files there and keep them")
    ap.add_argument("-v", "--verbose", action="store_true", help="list every kernel, not only the failing ones")
    args = ap.parse_args()
    if not hipcc():
        print("hipcc not found", file=sys.stderr)
        return 2
    outdir = args.keep or tempfile.mkdtemp(prefix="lds_ring_")
    os.makedirs(outdir, exist_ok=True)
    bad = 0
    try:
        for unit in units():
            for label, drains, counted, missing in check_unit(compile_to_asm(unit, outdir)):
                fail = drains > 0 or missing
                bad += bool(fail)
                if fail or args.verbose:
                    print("%-5s %-22s %-40s vmcnt(0) before ds_read: %d   counted waits: %s%s"
                          % ("FAIL" if fail else "ok", unit, label, drains, counted, ("   missing: %s" % missing) if missing else ""))
    finally:
        if not args.keep:
            shutil.rmtree(outdir, ignore_errors=True)
    print("%d kernel(s) drain the LDS-DMA ring" % bad if bad else "every ring kernel keeps its tiles in flight")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
