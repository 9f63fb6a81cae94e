"""Caller-supplied and mined negatives of the fused link loss (include/hgin.h A18), host side (no GPU): the public
surface and the header's spec section exist, the two new entry points reject bad arguments before touching the device,
the Python layer refuses a malformed negative set before any launch, ``LinkPredictor`` mines when it says it does and
calls ``sampled_link_loss`` the way it says it does (fake model, fake graph, no device), and the bench tool's plan is
unchanged by ``--hard``."""
import ctypes
import importlib.util
import os

import pytest
import torch

_Q = ctypes.c_void_p(16)   # a non-NULL pointer that must never be dereferenced


def test_public_surface():
    import hgin
    from hgin import linkpred
    assert "hard_negatives" in hgin.__all__ and hgin.hard_negatives is linkpred.hard_negatives
    assert callable(hgin.LinkPredictor.mine)
    import inspect
    for fn in (linkpred.negative_edges, linkpred.link_loss, linkpred.sampled_link_loss, linkpred.link_ranks,
               linkpred.link_metrics, hgin.LinkPredictor.metrics):
        assert inspect.signature(fn).parameters["neg_dst"].default is None, fn.__name__
    sig = inspect.signature(hgin.LinkPredictor.__init__).parameters
    assert sig["hard"].default == 0 and sig["mine_every"].default == 1
    names = list(inspect.signature(linkpred.hard_negatives).parameters)
    assert names == ["z_src", "z_dst", "pos", "m", "known", "seed", "offset"]


def test_abi_13_and_the_header_section():
    import re

    from conftest import ROOT
    from hgin import _lib
    assert _lib.ABI_VERSION >= 13
    for name in ("hgin_link_loss_fwd_neg_f32", "hgin_link_rank_neg_f32"):
        assert name in _lib.exported_symbols()
    assert _lib.lib().hgin_abi_version() == _lib.ABI_VERSION
    text = open(os.path.join(ROOT, "include", "hgin.h")).read()
    assert int(re.search(r"#define HGIN_ABI_VERSION (\d+)", text).group(1)) >= 13
    a18 = text[text.index("A18"):]
    a18 = a18[:a18.index("---- A15")]
    for word in ("hgin_link_loss_fwd_neg_f32", "hgin_link_rank_neg_f32", "neg_dst", "K = k + m", "offset + e k",
                 "0.5 / (E K)", "coef[E + e K"):
        assert word in a18, word


def _fwd(lib, pos=_Q, E=4, k=2, n_dst=3, neg_dst=_Q, m=2, zs=_Q, zd=_Q, F=8, coef=_Q, neg=_Q, loss=_Q, ws=_Q,
         ws_bytes=1 << 20, objective=0, param=1.0):
    return lib.hgin_link_loss_fwd_neg_f32(pos, E, k, 1, 0, n_dst, neg_dst, m, zs, F, zd, F, F, coef, neg, loss, ws,
                                          ws_bytes, objective, param, None)


def _rank(lib, pos=_Q, E=4, k=2, n_dst=3, neg_dst=_Q, m=2, zs=_Q, zd=_Q, F=8, gt=_Q, eq=_Q):
    return lib.hgin_link_rank_neg_f32(pos, E, k, 1, 0, n_dst, neg_dst, m, zs, F, zd, F, F, gt, eq, None)


def test_argument_errors_do_not_touch_the_device():
    from hgin import _lib
    lib = _lib.lib()
    err = lib.hgin_last_error
    for call in (_fwd, _rank):
        assert call(lib, E=0) == -1 and b"E = 0" in err()
        assert call(lib, E=1 << 31) == -1 and b"E = " in err()
        assert call(lib, k=-1) == -1 and b"k = -1 must be >= 0" in err()
        assert call(lib, m=0) == -1 and b"m = 0 must be >= 1" in err()
        assert call(lib, m=-3) == -1 and b"m = -3 must be >= 1" in err()
        assert call(lib, E=1 << 20, k=1 << 10, m=1 << 10) == -1 and b"E * (k + m)" in err()
        assert call(lib, E=1 << 20, k=0, m=1 << 11) == -1 and b"E * (k + m)" in err()
        assert call(lib, n_dst=0) == -1 and b"n_dst" in err()
        assert call(lib, n_dst=1 << 31) == -1 and b"n_dst" in err()
        assert call(lib, F=1 << 24) == -1 and b"F " in err()
        assert call(lib, pos=None) == -1 and b"pos NULL" in err()
        assert call(lib, neg_dst=None) == -1 and b"neg_dst NULL" in err()
        assert call(lib, zs=None) == -1 and b"z_src NULL" in err()
        assert call(lib, zd=None) == -1 and b"z_dst NULL" in err()
        # k = 0 with m = 2 is a legal shape: it passes every size check, and the error that comes back is the later one
        assert call(lib, k=0, m=2, zd=None) == -1 and b"z_dst NULL" in err()
    assert _fwd(lib, coef=None) == -1 and b"coef NULL" in err()
    assert _fwd(lib, neg=None) == -1 and b"neg NULL" in err()
    assert _fwd(lib, loss=None) == -1 and b"loss NULL" in err()
    assert _fwd(lib, k=0, m=2, coef=None) == -1 and b"coef NULL" in err()
    assert _rank(lib, gt=None) == -1 and b"n_greater NULL" in err()
    assert _rank(lib, eq=None) == -1 and b"n_equal NULL" in err()
    assert _rank(lib, k=0, m=2, eq=None) == -1 and b"n_equal NULL" in err()
    for obj in range(4):
        assert _fwd(lib, objective=obj, ws_bytes=8) == -3 and b"workspace" in err()
        assert _fwd(lib, objective=obj, ws=None) == -3 and b"workspace" in err()
        assert _fwd(lib, objective=obj, k=0, m=2, ws_bytes=8) == -3 and b"workspace" in err()
    for bad in (-1, 4, 17):
        assert _fwd(lib, objective=bad) == -1 and b"objective" in err()
    for tau in (0.0, -0.5, float("nan"), float("inf")):
        assert _fwd(lib, objective=1, param=tau) == -1 and b"temperature" in err()
    for alpha in (-1.0, float("nan"), float("inf")):
        assert _fwd(lib, objective=3, param=alpha) == -1 and b"alpha" in err()
    # the existing entry points still refuse k = 0
    assert lib.hgin_link_loss_fwd_obj_f32(_Q, 4, 0, 1, 0, 3, _Q, 8, _Q, 8, 8, _Q, _Q, _Q, _Q, 1 << 20, 0, 1.0,
                                          None) == -1 and b"k = 0" in err()
    assert lib.hgin_link_rank_f32(_Q, 4, 0, 1, 0, 3, _Q, 8, _Q, 8, 8, _Q, _Q, None) == -1 and b"k = 0" in err()


def test_python_errors_before_any_launch():
    from hgin import linkpred
    z = torch.zeros(3, 4)
    pos = torch.zeros(2, 5, dtype=torch.long)
    good = torch.zeros(5, 2, dtype=torch.int32)
    fns = (lambda **kw: linkpred.sampled_link_loss(z, z, pos, 1, 0, **kw),
           lambda **kw: linkpred.link_loss(z, z, pos, 1, 0, **kw),
           lambda **kw: linkpred.link_ranks(z, z, pos, 1, 0, **kw),
           lambda **kw: linkpred.link_metrics(z, z, pos, 1, 0, **kw),
           lambda **kw: linkpred.negative_edges(pos, 3, 1, 0, **kw))
    for fn in fns:
        with pytest.raises(ValueError, match=r"neg_dst must be \[E, m\]"):
            fn(neg_dst=good.reshape(-1))                       # wrong rank
        with pytest.raises(ValueError, match=r"neg_dst must be \[E, m\]"):
            fn(neg_dst=good[:4])                               # wrong E
        with pytest.raises(ValueError, match=r"neg_dst must be \[E, m\]"):
            fn(neg_dst=good[:, :0])                            # m = 0
        with pytest.raises(TypeError, match="neg_dst must be an int32 or int64 tensor"):
            fn(neg_dst=good.float())
        with pytest.raises(TypeError, match="neg_dst must be an int32 or int64 tensor"):
            fn(neg_dst=[[0, 1]] * 5)
        with pytest.raises(RuntimeError, match="no CPU fallback"):   # well-formed, but nothing here runs on the host
            fn(neg_dst=good)
    # k = 0 is an error without a set, k < 0 with one
    for fn in (linkpred.sampled_link_loss, linkpred.link_ranks, linkpred.link_metrics):
        with pytest.raises(ValueError, match="k >= 1"):
            fn(z, z, pos, 0, 0)
        with pytest.raises(ValueError, match="k >= 0"):
            fn(z, z, pos, -1, 0, neg_dst=good)
        with pytest.raises(RuntimeError, match="no CPU fallback"):   # k = 0 with a set gets as far as the device check
            fn(z, z, pos, 0, 0, neg_dst=good)
    for m in (0, 129, -1):
        with pytest.raises(ValueError, match="1 <= m <= 128"):
            linkpred.hard_negatives(z, z, pos, m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        linkpred.hard_negatives(z, z, pos, 2)


class _Model:
    training = True

    def __init__(self):
        self.encodes = 0

    def encode(self, x, e):
        self.encodes += 1
        return {"a": torch.full((3, 2), float(self.encodes)), "b": torch.full((4, 2), -float(self.encodes))}

    def eval(self):
        self.training = False

    def train(self, mode=True):
        self.training = mode


class _Graph:
    edge_index = {("a", "to", "b"): torch.zeros(2, 6, dtype=torch.long)}

    def x_dict(self):
        return {}

    def edge_index_dict(self):
        return {}


def test_predictor_argument_errors():
    from hgin import linkpred
    rel = ("a", "to", "b")
    with pytest.raises(ValueError, match="hard"):
        linkpred.LinkPredictor(_Model(), rel, 1, 0, hard=129)
    with pytest.raises(ValueError, match="hard"):
        linkpred.LinkPredictor(_Model(), rel, 1, 0, hard=-1)
    with pytest.raises(ValueError, match="k >= 1"):
        linkpred.LinkPredictor(_Model(), rel, 0, 0)
    with pytest.raises(ValueError, match="k >= 1"):
        linkpred.LinkPredictor(_Model(), rel, -1, 0, hard=2)
    with pytest.raises(ValueError, match="mine_every"):
        linkpred.LinkPredictor(_Model(), rel, 1, 0, hard=2, mine_every=-1)
    pred = linkpred.LinkPredictor(_Model(), rel, 0, 0, hard=128)
    assert (pred.k, pred.hard, pred.mine_every, pred.neg_dst) == (0, 128, 1, None)
    pred = linkpred.LinkPredictor(_Model(), rel, 3, 0)
    assert (pred.hard, pred.mine_every, pred.neg_dst) == (0, 1, None)
    with pytest.raises(ValueError, match="hard = 0"):
        pred.mine(_Graph())


def test_predictor_without_hard_makes_the_unchanged_positional_call(monkeypatch):
    from hgin import linkpred
    seen = []

    def fake(*args):   # a keyword would be a TypeError here
        seen.append(args)
        return "loss"

    def no_mining(*args, **kw):
        raise AssertionError("hard = 0 must not mine")

    monkeypatch.setattr(linkpred, "sampled_link_loss", fake)
    monkeypatch.setattr(linkpred, "hard_negatives", no_mining)
    pred = linkpred.LinkPredictor(_Model(), ("a", "to", "b"), 4, 9, objective="bpr")
    g = _Graph()
    assert pred.loss(g, step=2) == "loss"
    (args,) = seen
    assert len(args) == 9 and args[2] is g.edge_index[("a", "to", "b")]
    assert args[3:] == (4, 9, 2 * 6 * 4, "bpr", 1.0, 1.0)
    assert pred.neg_dst is None


def test_predictor_mines_every_third_step_and_passes_the_set_by_keyword(monkeypatch):
    from hgin import linkpred
    calls, mined = [], []

    def fake_loss(*args, **kw):
        calls.append((args, kw))
        return "loss"

    def fake_mine(z_src, z_dst, pos, m, known=None, seed=0, offset=0):
        assert not z_src.requires_grad and not z_dst.requires_grad
        mined.append(dict(z_src=z_src, z_dst=z_dst, pos=pos, m=m, known=known, seed=seed, offset=offset))
        return torch.full((int(pos.size(1)), m), len(mined), dtype=torch.int32)

    monkeypatch.setattr(linkpred, "sampled_link_loss", fake_loss)
    monkeypatch.setattr(linkpred, "hard_negatives", fake_mine)
    model, g = _Model(), _Graph()
    rel = ("a", "to", "b")
    pred = linkpred.LinkPredictor(model, rel, 4, 9, objective="softmax", temperature=0.5, hard=2, mine_every=3)
    for step in range(8):
        assert pred.loss(g, step=step) == "loss"
    assert model.encodes == 8                      # mining costs no second encode
    assert len(mined) == 3                         # steps 0, 3 and 6 only
    for j, step in enumerate((0, 3, 6)):
        c = mined[j]
        assert c["m"] == 2 and c["pos"] is g.edge_index[rel] and c["known"] is g.edge_index[rel]
        assert float(c["z_src"][0, 0]) == step + 1 and float(c["z_dst"][0, 0]) == -(step + 1)   # that step's embeddings
    for step, (args, kw) in enumerate(calls):
        assert len(args) == 9 and args[3:] == (4, 9, step * 6 * 4, "softmax", 0.5, 1.0)
        assert float(args[0][0, 0]) == step + 1
        assert list(kw) == ["neg_dst"] and kw["neg_dst"] is pred_sets(step, calls)
        assert int(kw["neg_dst"][0, 0]) == step // 3 + 1 and tuple(kw["neg_dst"].shape) == (6, 2)
    assert pred.neg_dst is calls[-1][1]["neg_dst"]

    # other positives: no set exists for them, so they are mined whatever the step
    other = torch.zeros(2, 5, dtype=torch.long)
    pred.loss(g, pos=other, step=7)
    assert len(mined) == 4 and mined[3]["pos"] is other and tuple(pred.neg_dst.shape) == (5, 2)

    # mine_every = 0: mined once (no set yet), then only by mine()
    pred = linkpred.LinkPredictor(model, rel, 0, 9, hard=3, mine_every=0)
    del mined[:], calls[:]
    for step in range(4):
        pred.loss(g, step=step)
    assert len(mined) == 1 and all(kw["neg_dst"] is pred.neg_dst for _, kw in calls)
    assert all(args[3:6] == (0, 9, 0) for args, _ in calls)    # k = 0: offset step * E * 0
    before, n_enc = pred.neg_dst, model.encodes
    model.training = True
    got = pred.mine(g)
    assert got is pred.neg_dst and got is not before and len(mined) == 2 and model.encodes == n_enc + 1
    assert model.training and mined[1]["known"] is g.edge_index[rel] and mined[1]["m"] == 3
    known = torch.zeros(2, 9, dtype=torch.long)
    pred.mine(g, pos=other, known=known)
    assert mined[2]["known"] is known and mined[2]["pos"] is other


def pred_sets(step, calls):
    """The set a step must have used: the one its mining step (0, 3, 6) passed."""
    return calls[step - step % 3][1]["neg_dst"]


def test_predictor_metrics_pass_an_evaluation_set_through(monkeypatch):
    from hgin import linkpred
    seen = []

    def fake(*args, **kw):
        seen.append((args, kw))
        return {}

    monkeypatch.setattr(linkpred, "link_metrics", fake)
    g = _Graph()
    pred = linkpred.LinkPredictor(_Model(), ("a", "to", "b"), 4, 9)
    pred.metrics(g)
    ev = torch.zeros(6, 3, dtype=torch.int64)
    pred.metrics(g, neg_dst=ev)
    assert len(seen[0][0]) == 5 and seen[0][1] == {}
    assert len(seen[1][0]) == 5 and list(seen[1][1]) == ["neg_dst"] and seen[1][1]["neg_dst"] is ev


def _tool():
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("bench_linkpred", os.path.join(ROOT, "tools", "bench_linkpred.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_bench_tool_hard_option_leaves_the_plan_alone(capsys):
    tool = _tool()
    shapes = tool.plan(["cfg2", "cfg3"], [1, 4], 1.0)
    assert [(s["config"], s["k"]) for s in shapes] == [("cfg2", 1), ("cfg2", 4), ("cfg3", 1), ("cfg3", 4)]
    assert sorted(shapes[0]) == ["E", "F", "config", "fwd_algorithmic_bytes", "k", "n_dst", "n_src",
                                 "rank_algorithmic_bytes", "scale"]
    if not torch.cuda.is_available():
        rc = tool.main(["--configs", "cfg1", "--scale", "0.1", "--k", "1"])
        plain = capsys.readouterr().err
        rc_hard = tool.main(["--configs", "cfg1", "--scale", "0.1", "--k", "1", "--hard", "3"])
        hard = capsys.readouterr().err
        assert rc == rc_hard == 2 and "no HIP device" in hard
        assert [ln for ln in hard.splitlines() if ln.startswith("plan:")] == \
               [ln for ln in plain.splitlines() if ln.startswith("plan:")]
    with pytest.raises(SystemExit):
        tool.main(["--configs", "cfg1", "--scale", "0.1", "--k", "1", "--hard", "0"])
    with pytest.raises(SystemExit):
        tool.main(["--configs", "cfg1", "--scale", "0.1", "--k", "1", "--hard", "129"])
