"""Link-prediction training path, host side (no GPU): the new entry points reject bad arguments before touching the
device, the public surface exists, and this file's float64 references of the sampled loss and of the ranking metrics
(the ones tests/test_gpu_linkpred.py checks the kernels against) give a hand-computed 2-edge case."""
import ctypes
import math

import numpy as np
import torch


# ---------------------------------------------------------------------------------------------------
# float64 references (shared with tests/test_gpu_linkpred.py)
# ---------------------------------------------------------------------------------------------------
def softplus64(x: torch.Tensor) -> torch.Tensor:
    return torch.clamp(x, min=0.0) + torch.log1p(torch.exp(-x.abs()))


def ref_loss(z_src: torch.Tensor, z_dst: torch.Tensor, pos: torch.Tensor, neg_dst, k: int) -> torch.Tensor:
    """0.5 mean_e softplus(-s_pos) + 0.5 mean_{e,j} softplus(s_neg) in the dtype of the embeddings (differentiable);
    negative e * k + j pairs pos[0, e] with neg_dst[e * k + j]."""
    nd = torch.as_tensor(np.asarray(neg_dst), dtype=torch.long)
    s_pos = (z_src[pos[0]] * z_dst[pos[1]]).sum(1)
    s_neg = (z_src[pos[0].repeat_interleave(k)] * z_dst[nd]).sum(1)
    return 0.5 * softplus64(-s_pos).mean() + 0.5 * softplus64(s_neg).mean()


def ref_loss_and_grads(z_src, z_dst, pos, neg_dst, k):
    """(loss, g_src, g_dst) in float64 on the CPU."""
    zs = z_src.detach().cpu().double().requires_grad_(True)
    zd = z_dst.detach().cpu().double().requires_grad_(True)
    loss = ref_loss(zs, zd, pos.cpu(), neg_dst, k)
    loss.backward()
    return loss.detach(), zs.grad, zd.grad


def ref_ranks(s_pos: np.ndarray, s_neg: np.ndarray, k: int):
    """(n_greater, n_equal) per positive from its score and its k negatives' scores ([E], [E * k])."""
    sn = np.asarray(s_neg).reshape(-1, k)
    sp = np.asarray(s_pos).reshape(-1, 1)
    return (sn > sp).sum(1).astype(np.int64), (sn == sp).sum(1).astype(np.int64)


def ref_metrics(n_greater: np.ndarray, n_equal: np.ndarray, k: int) -> dict:
    gt, eq = np.asarray(n_greater, np.float64), np.asarray(n_equal, np.float64)
    rank = 1.0 + gt + 0.5 * eq
    out = {"auc": 1.0 - (gt.sum() + 0.5 * eq.sum()) / (gt.size * k), "mrr": float((1.0 / rank).mean())}
    for K in (1, 3, 10):
        out[f"hits@{K}"] = float((rank <= K).mean())
    return out


# ---------------------------------------------------------------------------------------------------
def _sp(x):
    return max(x, 0.0) + math.log1p(math.exp(-abs(x)))


def _sig(x):
    return 1.0 / (1.0 + math.exp(-x))


def test_reference_on_a_hand_computed_two_edge_case():
    """z_src = [[1, 0], [0, 2]], z_dst = [[1, 1], [3, -1]], positives (0 -> 0), (1 -> 1), k = 2 with negatives
    (0 -> 1), (0 -> 0), (1 -> 0), (1 -> 1): s_pos = [1, -2], s_neg = [3, 1, 2, -2]."""
    zs = torch.tensor([[1.0, 0.0], [0.0, 2.0]])
    zd = torch.tensor([[1.0, 1.0], [3.0, -1.0]])
    pos = torch.tensor([[0, 1], [0, 1]])
    neg_dst, k = [1, 0, 0, 1], 2
    want = 0.25 * (_sp(-1.0) + _sp(2.0)) + 0.125 * (_sp(3.0) + _sp(1.0) + _sp(2.0) + _sp(-2.0))
    loss, g_src, g_dst = ref_loss_and_grads(zs, zd, pos, neg_dst, k)
    assert abs(float(loss) - want) < 1e-14
    assert abs(want - 1.43701056) < 1e-7   # 0.25 * 2.44018970 + 0.125 * 6.61570506
    cp = [0.25 * (_sig(1.0) - 1.0), 0.25 * (_sig(-2.0) - 1.0)]
    cn = [0.125 * _sig(3.0), 0.125 * _sig(1.0), 0.125 * _sig(2.0), 0.125 * _sig(-2.0)]
    zdn = zd.double().numpy()
    zsn = zs.double().numpy()
    want_src = np.stack([cp[0] * zdn[0] + cn[0] * zdn[1] + cn[1] * zdn[0],
                         cp[1] * zdn[1] + cn[2] * zdn[0] + cn[3] * zdn[1]])
    want_dst = np.stack([cp[0] * zsn[0] + cn[1] * zsn[0] + cn[2] * zsn[1],
                         cp[1] * zsn[1] + cn[0] * zsn[0] + cn[3] * zsn[1]])
    assert np.allclose(g_src.numpy(), want_src, rtol=0, atol=1e-15)
    assert np.allclose(g_dst.numpy(), want_dst, rtol=0, atol=1e-15)

    gt, eq = ref_ranks(np.array([1, -2]), np.array([3, 1, 2, -2]), k)
    assert gt.tolist() == [1, 1] and eq.tolist() == [1, 1]
    m = ref_metrics(gt, eq, k)   # ranks 2.5 and 2.5
    assert m["auc"] == 1.0 - 3.0 / 4.0 and abs(m["mrr"] - 0.4) < 1e-15
    assert m["hits@1"] == 0.0 and m["hits@3"] == 1.0 and m["hits@10"] == 1.0
    m = ref_metrics(np.array([0, 4, 9]), np.array([0, 0, 2]), 12)   # ranks 1, 5, 11
    assert abs(m["auc"] - (1.0 - 14.0 / 36.0)) < 1e-15 and abs(m["mrr"] - (1 + 0.2 + 1 / 11) / 3) < 1e-15
    assert m["hits@1"] == 1 / 3 and m["hits@3"] == 1 / 3 and m["hits@10"] == 2 / 3


def test_public_surface():
    import hgin
    from hgin import linkpred, train
    for cls in (hgin.HetroGIN, hgin.HetroGAT):
        assert callable(getattr(cls, "encode"))
    assert hgin.HetroGAT.encode is hgin.HetroGIN.encode
    for name in ("LinkPredictor", "sampled_link_loss", "link_ranks", "link_metrics", "link_train_step"):
        assert name in hgin.__all__ and getattr(hgin, name) is not None
    assert hgin.sampled_link_loss is linkpred.sampled_link_loss and hgin.link_train_step is train.link_train_step
    # the baseline pieces the fused path is checked against are still there
    for name in ("link_loss", "dot_decode", "negative_edges", "sample_negative_dst"):
        assert callable(getattr(linkpred, name))


def test_fused_path_refuses_host_tensors_and_other_dtypes():
    import pytest

    from hgin import linkpred
    z = torch.zeros(3, 4)
    pos = torch.zeros(2, 2, dtype=torch.long)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        linkpred.sampled_link_loss(z, z, pos, 1, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        linkpred.link_ranks(z, z, pos, 1, 0)


def test_bench_tool_plans_shapes_on_the_cpu_and_fails_without_a_gpu(capsys):
    import importlib.util
    import os

    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("bench_linkpred", os.path.join(ROOT, "tools", "bench_linkpred.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    shapes = tool.plan(["cfg2", "cfg3"], [1, 4], 1.0)
    assert [(s["config"], s["k"]) for s in shapes] == [("cfg2", 1), ("cfg2", 4), ("cfg3", 1), ("cfg3", 4)]
    s = shapes[3]
    assert (s["n_src"], s["n_dst"], s["E"], s["F"]) == (6_000_000, 3_000_000, 30_000_000, 256)
    E, k, F = s["E"], 4, 256
    assert s["fwd_algorithmic_bytes"] == E * F * 4 + (1 + k) * E * F * 4 + (1 + k) * E * 4 + 2 * E * k * 8 + 2 * E * 8
    assert shapes[0]["F"] == 128 and shapes[0]["E"] == 3_000_000
    if not torch.cuda.is_available():
        rc = tool.main(["--configs", "cfg1", "--scale", "0.1", "--k", "1"])
        err = capsys.readouterr().err
        assert rc == 2 and "no HIP device" in err and '"E": 200' in err


_Q = ctypes.c_void_p(16)   # a non-NULL pointer that must never be dereferenced


def _fwd(lib, pos=_Q, E=4, k=2, n_dst=3, zs=_Q, zd=_Q, F=8, coef=_Q, neg=_Q, loss=_Q, ws=_Q, ws_bytes=1 << 20):
    return lib.hgin_link_loss_fwd_f32(pos, E, k, 1, 0, n_dst, zs, F, zd, F, F, coef, neg, loss, ws, ws_bytes, None)


def _rank(lib, pos=_Q, E=4, k=2, n_dst=3, zs=_Q, zd=_Q, F=8, gt=_Q, eq=_Q):
    return lib.hgin_link_rank_f32(pos, E, k, 1, 0, n_dst, zs, F, zd, F, F, gt, eq, None)


def test_argument_errors_do_not_touch_the_device():
    from hgin import _lib
    lib = _lib.lib()
    err = lib.hgin_last_error
    for call in (_fwd, _rank):
        assert call(lib, E=0) == -1 and b"E = 0" in err()
        assert call(lib, k=0) == -1 and b"k = 0" in err()
        assert call(lib, n_dst=0) == -1 and b"n_dst" in err()
        assert call(lib, n_dst=1 << 31) == -1 and b"n_dst" in err()
        assert call(lib, E=1 << 20, k=1 << 11) == -1 and b"E * k" in err()
        assert call(lib, E=1 << 31) == -1 and b"E = " in err()
        assert call(lib, F=1 << 24) == -1 and b"F " in err()
        assert call(lib, pos=None) == -1 and b"pos NULL" in err()
        assert call(lib, zs=None) == -1 and b"z_src NULL" in err()
        assert call(lib, zd=None) == -1 and b"z_dst NULL" in err()
    assert _fwd(lib, coef=None) == -1 and b"coef NULL" in err()
    assert _fwd(lib, neg=None) == -1 and b"neg NULL" in err()
    assert _fwd(lib, loss=None) == -1 and b"loss NULL" in err()
    assert _fwd(lib, ws_bytes=8) == -3 and b"workspace" in err()
    assert _rank(lib, gt=None) == -1 and b"n_greater NULL" in err()
    assert _rank(lib, eq=None) == -1 and b"n_equal NULL" in err()

    sz = ctypes.c_size_t(0)
    assert lib.hgin_link_loss_workspace_size(1000, ctypes.byref(sz)) == 0 and sz.value >= 4
    assert lib.hgin_link_loss_workspace_size(1000, None) == -1
    assert lib.hgin_link_loss_workspace_size(0, ctypes.byref(sz)) == -1

    def bsrc(rowptr=_Q, n_src=5, E=4, k=2, g=_Q, coef=_Q, neg=_Q, zd=_Q, F=8, out=_Q):
        return lib.hgin_link_loss_bwd_src_f32(rowptr, _Q, _Q, n_src, E, k, g, coef, neg, zd, F, F, out, F, None)

    assert bsrc(E=0) == -1 and b"E must" in err()
    assert bsrc(k=0) == -1 and b"k must" in err()
    assert bsrc(E=1 << 20, k=1 << 11) == -1 and b"E * k" in err()
    assert bsrc(n_src=0) == -1 and b"n_src" in err()
    assert bsrc(rowptr=None) == -1 and b"rowptr" in err()
    assert bsrc(g=None) == -1 and b"g / coef / neg NULL" in err()
    assert bsrc(zd=None) == -1 and b"z_dst" in err()
    assert bsrc(out=None) == -1 and b"g_src" in err()

    def bdst(prow=_Q, nrow=_Q, n_dst=5, E=4, g=_Q, zs=_Q, F=8, out=_Q):
        return lib.hgin_link_loss_bwd_dst_f32(prow, _Q, _Q, nrow, _Q, _Q, n_dst, E, g, _Q, zs, F, F, out, F, None)

    assert bdst(E=0) == -1 and b"E must" in err()
    assert bdst(n_dst=0) == -1 and b"n_dst" in err()
    assert bdst(prow=None) == -1 and b"pos_rowptr" in err()
    assert bdst(nrow=None) == -1 and b"neg_rowptr" in err()
    assert bdst(g=None) == -1 and b"g / coef NULL" in err()
    assert bdst(zs=None) == -1 and b"z_src" in err()
    assert bdst(out=None) == -1 and b"g_dst" in err()
