"""Writes tests/golden/wsd_tail_sha256.json: SHA-256 of the outputs of every case of tests/test_gpu_wsd_tail.py
(g_w, g_a, g_b, g_z of mlp_bwd_w and the plain gemm_tn on g_z), with the CU count they were recorded at.  Run on a
GPU against a build of the commit whose bits are to be kept (the parent of the change under test):

    python tests/golden/make_wsd_tail_sha256.py [--lib path/to/that/libhgin.so] [--out FILE]
"""
import argparse
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnn-link-prediction_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="load this libhgin.so (same ABI) instead of the in-tree build")
    ap.add_argument("--out", default=os.path.join(HERE, "wsd_tail_sha256.json"))
    args = ap.parse_args()
    from hgin import _lib
    if args.lib:
        _lib.build = lambda *a, **k: os.path.abspath(args.lib)
    spec = importlib.util.spec_from_file_location("wsd_tail", os.path.join(ROOT, "tests", "test_gpu_wsd_tail.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    cases = t.all_case_hashes()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"cus": t.grid(), "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(cases)} cases -> {args.out}")


if __name__ == "__main__":
    main()
