"""Objectives of the fused link loss (include/hgin.h A17), host side (no GPU): this file's float64 reference of the
four objectives (the one tests/test_gpu_linkobj.py checks the kernels against), its closed forms, the spec table's
coefficients against autograd, and the argument errors that must be raised before any launch."""
import ctypes
import math

import numpy as np
import pytest
import torch

from test_linkpred_host import ref_loss, softplus64

OBJECTIVES = ("bce", "softmax", "bpr", "selfadv")


# ---------------------------------------------------------------------------------------------------
# reference (shared with tests/test_gpu_linkobj.py)
# ---------------------------------------------------------------------------------------------------
def ref_scores(z_src, z_dst, pos, neg_dst, k):
    """(s_pos [E], s_neg [E, k]) in the dtype of the embeddings (differentiable); negative e * k + j pairs
    pos[0, e] with neg_dst[e * k + j].  Pair by pair, as tests/test_linkpred_host.py::ref_loss forms them (the
    backward is then a sum of coefficient * row products, the expression the kernels evaluate); past 2^22 gathered
    elements the scores are read off the full [n_src, n_dst] product instead, which keeps a large E small."""
    nd = torch.as_tensor(np.asarray(neg_dst), dtype=torch.long)
    if pos.size(1) * k * z_src.size(1) > 2**22:
        full = z_src @ z_dst.t()
        return full[pos[0], pos[1]], full[pos[0].repeat_interleave(k), nd].reshape(-1, k)
    s_pos = (z_src[pos[0]] * z_dst[pos[1]]).sum(1)
    s_neg = (z_src[pos[0].repeat_interleave(k)] * z_dst[nd]).sum(1)
    return s_pos, s_neg.reshape(-1, k)


def softplus_ref(x: torch.Tensor) -> torch.Tensor:
    """log(1 + exp(x)) without overflow whose autograd derivative is sigmoid(x) everywhere, 1 / 2 at x = 0 included
    (bpr meets x = 0 exactly whenever a drawn negative is the positive's own destination)."""
    return torch.logaddexp(x, torch.zeros_like(x))


def obj_from_scores(s_pos, s_neg, objective, param):
    """The loss of include/hgin.h A17's table as a function of the pair scores."""
    if objective == "bce":
        return 0.5 * softplus64(-s_pos).mean() + 0.5 * softplus64(s_neg).mean()
    if objective == "softmax":
        x = torch.cat([s_pos.unsqueeze(1), s_neg], 1) / param
        return (torch.logsumexp(x, 1) - x[:, 0]).mean()
    if objective == "bpr":
        return softplus_ref(s_neg - s_pos.unsqueeze(1)).mean()
    if objective == "selfadv":
        p = torch.softmax(param * s_neg, 1).detach()   # a constant, as in the paper
        return 0.5 * (softplus_ref(-s_pos) + (p * softplus_ref(s_neg)).sum(1)).mean()
    raise AssertionError(objective)


def ref_obj_loss(z_src, z_dst, pos, neg_dst, k, objective, param):
    return obj_from_scores(*ref_scores(z_src, z_dst, pos, neg_dst, k), objective, param)


def ref_obj_loss_and_grads(zs, zd, pos, neg_dst, k, objective, param, dtype=torch.float64):
    """(loss, g_src, g_dst) on the CPU through autograd, float64 unless ``dtype`` says otherwise (float32: the
    restatement that shows what a careful single-precision evaluation of the same expression can reach)."""
    a = zs.detach().cpu().to(dtype).requires_grad_(True)
    b = zd.detach().cpu().to(dtype).requires_grad_(True)
    loss = ref_obj_loss(a, b, pos.cpu(), neg_dst, k, objective, param)
    loss.backward()
    return loss.detach(), a.grad, b.grad


def spec_coefficients(s_pos, s_neg, objective, param):
    """(c_pos [E], c_neg [E, k]) = d loss / d score as include/hgin.h A17's table states them."""
    E, k = s_neg.shape
    sig = torch.sigmoid
    if objective == "bce":
        return -0.5 * sig(-s_pos) / E, 0.5 * sig(s_neg) / (E * k)
    if objective == "softmax":
        p = torch.softmax(torch.cat([s_pos.unsqueeze(1), s_neg], 1) / param, 1)
        return (p[:, 0] - 1.0) / (param * E), p[:, 1:] / (param * E)
    if objective == "bpr":
        d = sig(s_neg - s_pos.unsqueeze(1)) / (E * k)
        return -d.sum(1), d
    p = torch.softmax(param * s_neg, 1)
    return -0.5 * sig(-s_pos) / E, 0.5 * p * sig(s_neg) / E


# ---------------------------------------------------------------------------------------------------
def _toy(n_dst, k, E=23, n_src=7, F=5, seed=3):
    g = torch.Generator().manual_seed(seed + n_dst)
    pos = torch.stack([torch.randint(0, n_src, (E,), generator=g), torch.randint(0, n_dst, (E,), generator=g)])
    zs = torch.randn(n_src, F, generator=g, dtype=torch.float64)
    zd = torch.randn(n_dst, F, generator=g, dtype=torch.float64)
    nd = torch.randint(0, n_dst, (E * k,), generator=g).numpy()
    return pos, zs, zd, nd


@pytest.mark.parametrize("k", [1, 3, 4])
def test_closed_forms_at_one_destination(k):
    """n_dst = 1: every score of a positive is the same number, so softmax = log(k + 1) at any temperature,
    bpr = log 2, and selfadv at alpha = 0 (p = 1 / k) is the bce reference."""
    pos, zs, zd, nd = _toy(1, k)
    for tau in (1.0, 0.25):
        assert abs(float(ref_obj_loss(zs, zd, pos, nd, k, "softmax", tau)) - math.log(k + 1)) < 1e-12
    assert abs(float(ref_obj_loss(zs, zd, pos, nd, k, "bpr", 0.0)) - math.log(2.0)) < 1e-12
    want = float(ref_loss(zs, zd, pos, nd, k))
    assert abs(float(ref_obj_loss(zs, zd, pos, nd, k, "selfadv", 0.0)) - want) < 1e-12
    assert abs(float(ref_obj_loss(zs, zd, pos, nd, k, "bce", 0.0)) - want) < 1e-15
    # and at any n_dst alpha = 0 is bce as a function
    pos, zs, zd, nd = _toy(9, k)
    assert abs(float(ref_obj_loss(zs, zd, pos, nd, k, "selfadv", 0.0)) - float(ref_loss(zs, zd, pos, nd, k))) < 1e-12


@pytest.mark.parametrize("objective,param", [("bce", 0.0), ("softmax", 1.0), ("softmax", 0.25), ("bpr", 0.0),
                                             ("selfadv", 0.0), ("selfadv", 1.0), ("selfadv", 4.0)])
@pytest.mark.parametrize("k", [1, 5])
def test_spec_table_coefficients_are_autograds(objective, param, k):
    pos, zs, zd, nd = _toy(9, k)
    s_pos, s_neg = ref_scores(zs, zd, pos, nd, k)
    s_pos, s_neg = s_pos.detach().requires_grad_(True), s_neg.detach().requires_grad_(True)
    obj_from_scores(s_pos, s_neg, objective, param).backward()
    c_pos, c_neg = spec_coefficients(s_pos.detach(), s_neg.detach(), objective, param)
    assert float((s_pos.grad - c_pos).abs().max()) < 1e-12
    assert float((s_neg.grad - c_neg).abs().max()) < 1e-12
    if objective in ("softmax", "bpr"):   # a positive's coefficients sum to zero
        assert float((c_pos + c_neg.sum(1)).abs().max()) < 1e-15


def test_softmax_and_selfadv_do_not_overflow_in_the_reference():
    s_pos = torch.tensor([800.0, -900.0], dtype=torch.float64)
    s_neg = torch.tensor([[900.0, -700.0], [-950.0, 1000.0]], dtype=torch.float64)
    assert abs(float(obj_from_scores(s_pos, s_neg, "softmax", 1.0)) - (100.0 + 1900.0) / 2) < 1e-9
    assert abs(float(obj_from_scores(s_pos, s_neg, "bpr", 0.0)) - (100.0 + 1900.0) / 4) < 1e-9
    assert abs(float(obj_from_scores(s_pos, s_neg, "selfadv", 1.0)) - 0.25 * (0.0 + 900.0 + 900.0 + 1000.0)) < 1e-9


# ---------------------------------------------------------------------------------------------------
# argument errors, without a device
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kwargs", [dict(objective="hinge"), dict(objective=None), dict(objective="softmax", temperature=0.0),
                                    dict(objective="softmax", temperature=-1.0), dict(alpha=-1.0),
                                    dict(objective="selfadv", alpha=-1.0), dict(temperature=float("nan")),
                                    dict(objective="selfadv", alpha=float("nan")),
                                    dict(objective="softmax", temperature=float("inf")), dict(alpha=float("inf"))])
def test_bad_objective_arguments_raise_value_error_before_any_launch(kwargs):
    from hgin import linkpred
    z = torch.zeros(3, 4)
    pos = torch.zeros(2, 2, dtype=torch.long)
    for fn in (linkpred.sampled_link_loss, linkpred.link_loss):
        with pytest.raises(ValueError, match="objective|temperature|alpha"):
            fn(z, z, pos, 1, 0, **kwargs)

    class _Model:
        def encode(self, x, e):
            raise AssertionError("not reached")

    with pytest.raises(ValueError, match="objective|temperature|alpha"):
        linkpred.LinkPredictor(_Model(), ("a", "to", "b"), 1, 0, **kwargs)


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_host_tensors_are_still_refused(objective):
    from hgin import linkpred
    z = torch.zeros(3, 4)
    pos = torch.zeros(2, 2, dtype=torch.long)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        linkpred.sampled_link_loss(z, z, pos, 1, 0, objective=objective)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        linkpred.link_loss(z, z, pos, 1, 0, objective=objective)


def test_predictor_stores_and_passes_the_objective(monkeypatch):
    import hgin
    from hgin import linkpred
    assert hgin.LINK_OBJECTIVES == OBJECTIVES and "LINK_OBJECTIVES" in hgin.__all__
    seen = {}

    class _Model:
        def encode(self, x, e):
            return {"a": "za", "b": "zb"}

    class _Graph:
        edge_index = {("a", "to", "b"): torch.zeros(2, 6, dtype=torch.long)}

        def x_dict(self):
            return {}

        def edge_index_dict(self):
            return {}

    def fake(*args):
        seen["args"] = args
        return "loss"

    monkeypatch.setattr(linkpred, "sampled_link_loss", fake)
    pred = linkpred.LinkPredictor(_Model(), ("a", "to", "b"), 4, 9, objective="softmax", temperature=0.5)
    assert (pred.objective, pred.temperature, pred.alpha) == ("softmax", 0.5, 1.0)
    assert pred.loss(_Graph(), step=2) == "loss"
    assert seen["args"][0:2] == ("za", "zb") and seen["args"][3:] == (4, 9, 2 * 6 * 4, "softmax", 0.5, 1.0)
    pred = linkpred.LinkPredictor(_Model(), ("a", "to", "b"), 4, 9)
    assert (pred.objective, pred.temperature, pred.alpha) == ("bce", 1.0, 1.0)


# ---------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------
_Q = ctypes.c_void_p(16)   # a non-NULL pointer that must never be dereferenced


def _fwd_obj(lib, objective, param, pos=_Q, E=4, k=2, n_dst=3, zs=_Q, zd=_Q, F=8, coef=_Q, neg=_Q, loss=_Q, ws=_Q,
             ws_bytes=1 << 20):
    return lib.hgin_link_loss_fwd_obj_f32(pos, E, k, 1, 0, n_dst, zs, F, zd, F, F, coef, neg, loss, ws, ws_bytes,
                                          objective, param, None)


def test_abi_12_exports_the_objective_entry_point_and_checks_its_arguments():
    from hgin import _lib
    assert _lib.ABI_VERSION >= 12
    assert "hgin_link_loss_fwd_obj_f32" in _lib.exported_symbols()
    lib = _lib.lib()
    assert lib.hgin_abi_version() == _lib.ABI_VERSION
    err = lib.hgin_last_error
    for bad in (-1, 4, 17):
        assert _fwd_obj(lib, bad, 1.0) == -1 and b"objective" in err()
    for tau in (0.0, -0.5, float("nan"), float("inf")):
        assert _fwd_obj(lib, 1, tau) == -1 and b"temperature" in err()
    for alpha in (-1.0, float("nan"), float("inf")):
        assert _fwd_obj(lib, 3, alpha) == -1 and b"alpha" in err()
    # the checks of hgin_link_loss_fwd_f32, for every objective
    for obj in range(4):
        assert _fwd_obj(lib, obj, 1.0, E=0) == -1 and b"E = 0" in err()
        assert _fwd_obj(lib, obj, 1.0, k=0) == -1 and b"k = 0" in err()
        assert _fwd_obj(lib, obj, 1.0, n_dst=0) == -1 and b"n_dst" in err()
        assert _fwd_obj(lib, obj, 1.0, E=1 << 20, k=1 << 11) == -1 and b"E * k" in err()
        assert _fwd_obj(lib, obj, 1.0, F=1 << 24) == -1 and b"F " in err()
        assert _fwd_obj(lib, obj, 1.0, pos=None) == -1 and b"pos NULL" in err()
        assert _fwd_obj(lib, obj, 1.0, zs=None) == -1 and b"z_src NULL" in err()
        assert _fwd_obj(lib, obj, 1.0, zd=None) == -1 and b"z_dst NULL" in err()
        assert _fwd_obj(lib, obj, 1.0, coef=None) == -1 and b"coef NULL" in err()
        assert _fwd_obj(lib, obj, 1.0, neg=None) == -1 and b"neg NULL" in err()
        assert _fwd_obj(lib, obj, 1.0, loss=None) == -1 and b"loss NULL" in err()
        assert _fwd_obj(lib, obj, 1.0, ws_bytes=8) == -3 and b"workspace" in err()
        assert _fwd_obj(lib, obj, 1.0, ws=None) == -3 and b"workspace" in err()


def test_header_carries_the_spec_table():
    import os

    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "hgin.h")).read()
    assert _abi_in_header(text) >= 12
    a17 = text[text.index("A17"):]
    for word in ("HGIN_LINK_OBJ_SOFTMAX", "HGIN_LINK_OBJ_BPR", "HGIN_LINK_OBJ_SELFADV", "logsumexp", "tau", "alpha",
                 "hgin_link_loss_fwd_obj_f32"):
        assert word in a17, word


def _abi_in_header(text):
    import re
    return int(re.search(r"#define HGIN_ABI_VERSION (\d+)", text).group(1))


def test_bench_tool_lists_the_objectives():
    import importlib.util
    import os

    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("bench_linkpred", os.path.join(ROOT, "tools", "bench_linkpred.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.objectives_of("all") == list(OBJECTIVES)
    assert tool.objectives_of("bpr") == ["bpr"] and tool.objectives_of("bce") == ["bce"]
    if not torch.cuda.is_available():
        assert tool.main(["--configs", "cfg1", "--scale", "0.1", "--k", "1", "--objective", "all"]) == 2
