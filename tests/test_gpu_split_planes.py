"""Every fp32 split-mode GEMM form pinned to the exact three-plane oracles of tests/split_oracles.py, under each
process-static kernel switch set, each in a fresh child process (tests/split_child.py; a separate interpreter started
with subprocess, never an exec of this process):

  * default
  * tiled          HGIN_NT_WS=0 HGIN_TN_WS=0 HGIN_NT_WS32=0: the tiled kernels at the weight-stationary shapes
  * tiled_nobdma   the same plus HGIN_NT_BDMA=0: the 128-row tiles split B themselves
  * nopro          HGIN_WSD_PRO=0: the separate PReLU-backward pass ahead of the plain weight-stationary dW
  * mfma32         HGIN_F32_GEMM=mfma32: the exact-f32 MFMA kernels meet the same oracles, so the oracles are not tuned
                   to the split

A split product is a1b1 plus five minor terms (a3b1, a2b2, a1b3, a2b1, a1b2).  The float64 tolerance tests allow
1e-5 sum |a||b| and dense random operands carry ~6e-7 of accumulation noise, so neither sees a kernel that loses a
minor term (<= 1.6e-6); the bitwise tests compare kernels with each other or with recorded bytes.  Here the operands
are built so that the result is exactly representable and every minor term contributes to >= 99 % of the outputs of
some oracle (tests/test_split_planes_host.py prints the mutation table on the CPU), and every output tensor (y, z, c,
g_x_dst, g_w, g_z) must equal the float64 reference bit for bit; g_eps / g_b / g_a, sums over per-workgroup partials,
keep their 1e-5 forms.  NaN rows stand behind every row operand and poisoned rows behind every output.

Forms (tests/split_child.py: NT_FORMS, TN_FORMS) x rows x oracles; the kernel each case ran is asserted from the
launch trace (expected_kernels below, read from the dispatch of csrc/hgin_gemm_nt.hip / hgin_gemm_tn.hip), so a dispatch
change cannot quietly move a case onto another kernel."""
import json
import os
import subprocess
import sys
import tempfile

import pytest

import split_child as sc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

TILED = {"HGIN_NT_WS": "0", "HGIN_TN_WS": "0", "HGIN_NT_WS32": "0"}
SWITCHES = {"default": {}, "tiled": TILED, "tiled_nobdma": {**TILED, "HGIN_NT_BDMA": "0"},
            "nopro": {"HGIN_WSD_PRO": "0"}, "mfma32": {"HGIN_F32_GEMM": "mfma32"}}
FAMILIES = {"nt_ws": [n for n, f in sc.NT_FORMS.items() if f[4] == "ws"],
            "nt_tiled": [n for n, f in sc.NT_FORMS.items() if f[4] != "ws"],
            "tn_ws": [n for n, f in sc.TN_FORMS.items() if f[4] == "ws"],
            "tn_tiled": [n for n, f in sc.TN_FORMS.items() if f[4] != "ws"]}
# the weight-stationary NT launches of a form (default and nopro)
NT_WS_TAGS = {
    "fwd256_acc0_z0": ["k_wss_f32<EPI1,0,0>"], "fwd256_acc0_z1": ["k_wss_f32<EPI1,0,1>"],
    "fwd256_acc1_z0": ["k_wss_f32<EPI1,1,0>"], "fwd256_acc1_z1": ["k_wss_f32<EPI1,1,1>"],
    "cat512_z1": ["k_wss_f32<EPI5,0,0>", "k_wss_f32<EPI1,1,1,init>"],
    "cat512_z0": ["k_wss_f32<EPI5,0,0>", "k_wss_f32<EPI1,1,0,init>"],
    "cat512_z1_off256": ["k_wss_f32<EPI5,0,0>", "k_wss_f32<EPI1,1,1,init>"],
    "plain256_k256": ["k_wss_f32<EPI5,0,0>"], "plain256_k128": ["k_wss_f32<EPI5,0,0,K128>"],
    "comb256_gx0": ["k_wss_f32<EPI4,1,0>"], "comb256_gx1": ["k_wss_f32<EPI4,1,1>"],
    "comb256_prev": ["k_ws_f32<256,256,EPI4>"],
}
# the tiled kernel's tile where the form does not run a weight-stationary kernel.  use_bm64 takes the 64-row tile at
# every row count of the K = N = 256 forms used here (up to 96 G + 5 rows) and the 128-row one from 35 001 rows on
NT_TILE = {"t64x128_fwd": "64x128", "t128x128_lin_k256": "128x128", "t128x128_plain_k128": "128x128",
           "t128x128_comb_k128": "128x128", "t128x256_fwd_k384": "128x256", "t256x32_fwd": "256x32",
           "t256x32_fwd_n7": "256x32", "t_unclean_k100": "64x128", "t_misaligned_a": "64x128",
           "t_cat512_acc": "128x256"}
EPI = {"fwd": 1, "lin": 2, "plain": 0, "comb": 4}
_results = {}


def expected_kernels(name, switches, planes=True):
    """The GEMM launches of a form under a switch set (planes=False: hgin.ops passes no pre-split planes)."""
    split = switches != "mfma32"
    ws = switches in ("default", "nopro")
    bdma = planes and split and switches != "tiled_nobdma"
    mode = "split" if split else "mfma32"
    if name in sc.NT_FORMS:
        kind, N, K = sc.NT_FORMS[name][:3]
        if ws and name in NT_WS_TAGS:
            return NT_WS_TAGS[name]
        tile = NT_TILE.get(name, "64x128")
        if tile in ("128x128", "128x256"):      # the tiles that copy B from the pre-split planes by LDS-DMA
            tile, mode = (tile, "split_bdma") if bdma else ("128x128", mode)
        return [f"k_gemm_nt<EPI{EPI[kind]},{tile},{mode},N{N},K{K}>"]
    N, K1, K2, how, rows = sc.TN_FORMS[name]
    K = K1 + K2
    pro = switches != "nopro"
    if rows == "ws" and ws:
        kv = K if K < 512 else 256              # K = 512: two 256-column passes
        kern = "k_wsp_f32" if (N == 256 and kv == 256) else "k_wsd_f32"
        plain = [f"{kern}<{N},{kv}>"] * (2 if K == 512 else 1)
        if how == "plain" or not pro:
            return plain
        if K == 512 and N == 128:
            return ["k_wsd_f32<128,512,prelu_bwd_fused>"]
        return [f"{kern}<{N},{kv},prelu_bwd_fused>"] + plain[1:]
    if how == "fused_nogz":
        pre = "prelu_bwd_fused"
    else:       # g_z wanted: formed by the tiled kernel where its rows are 16-B aligned, else by a pass of its own
        pre = "prelu_bwd_fused+gz" if (how == "fused" and pro and N % 4 == 0) else "plain"
    return [f"k_gemm_tn_partial<{pre},{mode},N{N},K{K}>"]


def _run(name):
    if name in _results:
        return _results[name]
    env = {k: v for k, v in os.environ.items() if not k.startswith("HGIN_")}
    env.update(SWITCHES[name])
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "res.json")
        p = subprocess.run([sys.executable, os.path.join(HERE, "split_child.py"), out], env=env,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, f"{name}: child failed ({p.returncode})\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
        with open(out) as f:
            _results[name] = json.load(f)
    meta = _results[name].pop("_meta")
    assert meta["selfcheck"], "the child's comparison does not report a one-ulp difference"
    assert meta["env"] == SWITCHES[name], meta
    return _results[name]


def _cases(res, family):
    return {k: v for k, v in res.items() if k.split("/")[0] in FAMILIES[family]}


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("switches", sorted(SWITCHES))
def test_split_planes_exact(switches, family):
    """Every output of every case equals the float64 reference bit for bit; guards untouched."""
    cases = _cases(_run(switches), family)
    rows = {k.split("/")[0]: set() for k in cases}
    for k in cases:
        rows[k.split("/")[0]].add(k.split("/")[1])
    assert sorted(rows) == sorted(FAMILIES[family])
    for name, r in rows.items():                       # every row count and every oracle of every form ran
        form = (sc.NT_FORMS if name in sc.NT_FORMS else sc.TN_FORMS)[name]
        want = (3 if name in sc.NT_FORMS else 4) if form[4] == "ws" else (1 if name in sc.NT_FORMS else 2)
        oracles = sc.so.NT_ORACLES if name in sc.NT_FORMS else sc.so.TN_ORACLES
        assert len(r) == want and all(f"{name}/{m}/{o}" in cases for m in r for o in oracles), name
    failing = {k: v["fail"] for k, v in cases.items() if v["fail"]}
    assert not failing, f"{len(failing)} of {len(cases)} cases: {dict(list(failing.items())[:8])}"


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("switches", sorted(SWITCHES))
def test_split_planes_kernel_identity(switches, family):
    cases = _cases(_run(switches), family)
    assert cases
    for k, v in cases.items():
        assert v["kernels"] == expected_kernels(k.split("/")[0], switches), (switches, k, v["kernels"])


@pytest.mark.parametrize("switches", sorted(SWITCHES))
def test_split_planes_each_minor_term_is_isolated(switches):
    """The cases that ran isolate every minor term in >= 99 % of the outputs of some oracle, for NT and for TN (the
    mutation rows the child's references reported)."""
    res = _run(switches)
    for fam in ("nt_ws", "nt_tiled", "tn_ws", "tn_tiled"):
        cases = _cases(res, fam)
        for term in sc.so.MINOR:
            assert max(v["table"][term] for v in cases.values()) >= 0.99, (fam, term)


@pytest.mark.parametrize("switches", ["default", "tiled", "nopro"])
def test_nt_planes_equal_in_kernel_split(switches):
    """hgin_nt_planes_f32: the 128-row tiles fed pre-split B planes by LDS-DMA and the same tiles splitting B
    themselves give the same bits, and both are the oracle's."""
    cases = {k: v for k, v in _run(switches).items() if k.startswith("planes/")}
    assert len(cases) == 12
    for k, v in cases.items():
        _, name, _, how = k.split("/")
        assert not v["fail"], (k, v["fail"])
        assert v["kernels"] == expected_kernels(name, switches, planes=how == "with"), (k, v["kernels"])
        assert ("split_bdma" in v["kernels"][0]) == (how == "with")
