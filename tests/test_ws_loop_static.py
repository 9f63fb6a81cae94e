"""CPU-side static check of the steady-state loops of the fp32 weight-stationary GEMMs (tools/ws_loop_mix.py compiles
both GEMM sources to gfx950 assembly with the library's flags and counts each kernel's main loop): no packed fp32
VALU (v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32 issued beside MFMAs stall the matrix pipe) in the dW kernels
k_wsp_f32 / k_wsd_f32 and the dX kernel k_wss_f32<4, ...>, and no v_readfirstlane_b32 in the two dW kernels (their
LDS-DMA addresses are set up ahead of the loop).  Instruction totals are recorded in DESIGN.md, not asserted."""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mix():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ws_loop_mix.py"), "--json"], capture_output=True,
                       text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return json.loads(p.stdout)


pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and shutil.which("hipcc") is None,
                                reason="hipcc not available")


def test_dw_and_dx_loops_have_no_packed_f32(mix):
    dw = [k for k in mix if k.startswith(("k_wsp_f32<", "k_wsd_f32<"))]
    dx = [k for k in mix if k.startswith("k_wss_f32<4,")]
    assert len([k for k in dw if k.startswith("k_wsp_f32<")]) == 2 and len(dw) >= 8 and len(dx) >= 2, sorted(mix)
    for k in dw + dx:
        assert mix[k]["mfma"] > 0, (k, mix[k])   # the loop that was counted is the one with the products
        assert mix[k]["pk_f32"] == 0, (k, mix[k])


def test_dw_loops_have_no_readfirstlane(mix):
    for k in mix:
        if k.startswith(("k_wsp_f32<", "k_wsd_f32<")):
            assert mix[k]["readfirstlane"] == 0, (k, mix[k])
