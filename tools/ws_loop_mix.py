"""Instruction mix of the steady-state loop of every fp32 weight-stationary GEMM kernel (k_wss_f32 in
hgin_gemm_nt.hip; k_wsp_f32 / k_wsd_f32 in hgin_gemm_tn.hip) in the gfx950 assembly of the library's own flags
(hgin/_lib.py).  The steady-state loop is the depth-1 loop of the kernel that holds the most MFMAs (the
peeled start-up and tail iterations are straight-line code outside it).  Where a loop holds both stagger roles
(waves 0-3 and 4-7) one wave executes about half of every count.

    python tools/ws_loop_mix.py                  # compiles both sources, prints one table row per kernel
    python tools/ws_loop_mix.py --json           # the same as one JSON object {kernel: {column: count}}
    python tools/ws_loop_mix.py --asm a.s b.s    # count in assembly compiled elsewhere
    python tools/ws_loop_mix.py --flag=-fno-slp-vectorize   # with extra compiler flags (experiments)
"""
import argparse
import collections
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnn-link-prediction_amd", "csrc")
SRCS = [os.path.join(CSRC, f) for f in ("hgin_gemm_nt.hip", "hgin_gemm_tn.hip")]
KERNELS = r"k_ws(?:s|p|d)_f32"
PACKED_F32 = ("v_pk_add_f32", "v_pk_mul_f32", "v_pk_fma_f32")
COLUMNS = ("mfma", "valu", "pk_f32", "readfirstlane", "cndmask", "branch", "salu", "vmem", "lds")


def compile_asm(src, out, extra=()):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc, "-O3", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", *extra,   # hgin/_lib.py's flags
           "--offload-device-only", "-S", "-I", os.path.join(ROOT, "include"), "-o", out, src]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def classify(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_accvgpr"):
        return "accmov"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_waitcnt") or op in ("s_nop", "s_barrier", "s_setprio"):
        return "sync"
    if op.startswith("s_cbranch") or op.startswith("s_branch"):
        return "branch"
    if op.startswith("s_"):
        return "salu"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("ds_"):
        return "lds"
    return "other"


def demangle(names):
    out = names
    for filt in ("/opt/rocm/llvm/bin/llvm-cxxfilt", shutil.which("llvm-cxxfilt"), shutil.which("c++filt")):
        if not filt or not os.path.exists(filt):
            continue
        try:
            p = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True)
            out = p.stdout.split("\n")[:len(names)]
            break
        except (OSError, subprocess.CalledProcessError):
            pass
    res = []
    for n in out:
        n = re.sub(r"^void ", "", n.replace("hgin::(anonymous namespace)::", ""))
        res.append(re.sub(r"\(.*", "", n))
    return res


def loop_mix(asm):
    """{mangled kernel name: Counter of the steady-state loop}; 'ops' holds the per-opcode VALU counts."""
    res = {}
    for m in re.finditer(r"^(_ZN4hgin12_GLOBAL__N_1\d+%s\S*):" % KERNELS, asm, re.M):
        body = asm[m.end():asm.index(".Lfunc_end", m.end())].split("\n")
        spans = []
        for h, line in enumerate(body):
            if "Loop Header: Depth=1" not in line:
                continue
            lab = re.match(r"^\.LBB(\d+_\d+)", line)
            if not lab:
                continue
            tag = "Header=BB%s " % lab.group(1)
            inside = [n for n, t in enumerate(body) if tag in t + " "]
            e = (max(inside) if inside else h) + 1
            while e < len(body) and not body[e].startswith(".LBB"):
                e += 1
            spans.append((h, e))
        # a loop entered at two points (the compiler peels the first block's wait variant into the preheader) carries
        # no loop comment: without a commented loop that holds MFMAs, take the backward branches' spans
        if not any("v_mfma" in t for h, e in spans for t in body[h:e]):
            labels = {m2.group(1): n for n, t in enumerate(body) for m2 in [re.match(r"^(\.LBB\d+_\d+):", t)] if m2}
            for n, t in enumerate(body):
                m2 = re.match(r"\s+s_c?branch\S*\s+(\.LBB\d+_\d+)", t)
                if m2 and labels.get(m2.group(1), n) < n:
                    spans.append((labels[m2.group(1)], n + 1))
            spans.sort(key=lambda s: s[1] - s[0])
        best = None
        for h, e in spans:   # ties: the first in the text
            c, ops = collections.Counter(), collections.Counter()
            for t in body[h:e]:
                t = t.strip()
                if not t or t[0] in ";." or t.endswith(":"):
                    continue
                op = t.split()[0]
                c[classify(op)] += 1
                ops[op] += 1
            if best is None or c["mfma"] > best[0]["mfma"]:
                best = (c, ops)
        if best is None or not best[0]["mfma"]:
            continue
        c, ops = best
        row = {k: c[k] for k in ("mfma", "valu", "branch", "salu", "vmem", "lds")}
        row["pk_f32"] = sum(ops[o] for o in PACKED_F32)
        row["readfirstlane"] = ops["v_readfirstlane_b32"]
        row["cndmask"] = sum(n for o, n in ops.items() if o.startswith("v_cndmask"))
        row["packed_ops"] = {o: ops[o] for o in PACKED_F32 if ops[o]}
        res[m.group(1)] = row
    names = list(res)
    return dict(zip(demangle(names), (res[n] for n in names)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm", nargs="*", help="count in these assembly files instead of compiling")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--flag", action="append", default=[], help="extra hipcc flag (repeatable)")
    args = ap.parse_args()
    if args.asm:
        asm = "".join(open(f).read() for f in args.asm)
    else:
        with tempfile.TemporaryDirectory() as d:
            with ThreadPoolExecutor(2) as ex:
                outs = list(ex.map(lambda a: compile_asm(a[1], os.path.join(d, f"k{a[0]}.s"), args.flag),
                                   enumerate(SRCS)))
            asm = "".join(open(f).read() for f in outs)
    mix = loop_mix(asm)
    if args.json:
        print(json.dumps(mix))
        return 0
    print("| kernel | " + " | ".join(COLUMNS) + " |")
    print("|---|" + "---|" * len(COLUMNS))
    for k in sorted(mix):
        print(f"| `{k}` | " + " | ".join(str(mix[k][c]) for c in COLUMNS) + " |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
