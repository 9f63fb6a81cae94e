"""The first layer's data-input aggregate served from the per-tensor cache (ops.STATIC_AGG): everything a step
computes is bitwise what it computes with the switch off, the layer-0 aggregate launches are gone from the second step
on, every edit of the inputs forces a recompute, and refilled batch buffers are never cached.

Sizes (the two smallest at which the paths differ):
  (a) cfg1 (600 / 300 / 100 nodes, H = 8, L = 2): the narrow kernels.  cfg1's model slices the path and link features
      inside the model (divided_features off), so only the node features reach the first layer as the graph's own
      tensors: one cached launch (node -> link);
  (b) cfg3 x 2e-5 with two layers (120 / 60 / 20 nodes, 600 / 100 edges, width 256): the headline's K = 512 two-pass
      forward and dW with the cached tensor as their first operand, the last row block partial; all three feature
      tensors reach the first layer untouched: four cached launches."""
import dataclasses
import gc

import pytest
import torch

from hgin import HetroGIN, _lib, conv, ops
from hgin.data import CONFIGS, REL_PL, scaled_config, synthetic_graph
from hgin.train import train_step

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = {"a": (scaled_config(CONFIGS["cfg1"], 1.0, name="cfg1"), 1),
         "b": (dataclasses.replace(scaled_config(CONFIGS["cfg3"], 2e-5, name="cfg3-tiny"), layers=2), 4)}
AGG = ("k_aggregate", "k_agg_pipe", "k_long")


def _cfg(size, feat="f32"):
    cfg, cached = SIZES[size]
    return dataclasses.replace(cfg, feat_dtype=feat), cached


def _model(cfg):
    torch.manual_seed(1997)
    return HetroGIN(**cfg.model_kwargs({"link": cfg.f_link, "path": cfg.f_path, "node": cfg.f_node})).to(DEV)


def _snap(model, loss):
    return ([loss.detach().clone()] + [p.detach().clone() for p in model.parameters()] +
            [None if p.grad is None else p.grad.detach().clone() for p in model.parameters()])


def _same(a, b, what=""):
    assert len(a) == len(b), what
    for i, (u, v) in enumerate(zip(a, b)):
        assert (u is None) == (v is None), (what, i)
        if u is not None:
            assert u.dtype == v.dtype and torch.equal(u, v), (what, i)


def _split(kernels):
    agg = [t for t in kernels if t.startswith(AGG)]
    return agg, [t for t in kernels if not t.startswith(AGG)]


def _run(cfg, on, steps=4, layer_fn=True, between=None, prepare=None, capturable=False):
    """``steps`` train steps on a fresh graph and model with the switch ``on``: (per-step snapshots, per-step launch
    traces, graph).  ``prepare(graph)`` runs before the first step, ``between(i, graph)`` after step i."""
    was, was_fn = ops.STATIC_AGG, conv.LAYER_FN
    ops.STATIC_AGG, conv.LAYER_FN = on, layer_fn
    try:
        g = synthetic_graph(cfg, seed=0, device=DEV)
        if prepare is not None:
            prepare(g)
        model = _model(cfg)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, capturable=capturable)
        snaps, traces = [], []
        for i in range(steps):
            with _lib.trace_launches() as tr:
                loss = train_step(model, opt, g)
            snaps.append(_snap(model, loss))
            traces.append(tr.kernels)
            if between is not None:
                between(i, g)
        torch.cuda.synchronize()
        return snaps, traces, g
    finally:
        ops.STATIC_AGG, conv.LAYER_FN = was, was_fn


@pytest.mark.parametrize("layer_fn", [True, False])
@pytest.mark.parametrize("feat", ["f32", "bf16"])
@pytest.mark.parametrize("size", ["a", "b"])
def test_trajectory_on_off(size, feat, layer_fn):
    """Four train steps from the same seed: loss, every parameter and every gradient bitwise equal after each step."""
    cfg, _ = _cfg(size, feat)
    on, _, g = _run(cfg, True, layer_fn=layer_fn)
    off, _, g_off = _run(cfg, False, layer_fn=layer_fn)
    for i, (a, b) in enumerate(zip(on, off)):
        _same(a, b, f"step {i}")
    assert any(ops.static_cache(t) for t in g.x.values())          # the on run did go through the cache
    assert not any(ops.static_cache(t) for t in g_off.x.values())


@pytest.mark.parametrize("size", ["a", "b"])
def test_launches(size):
    """Step 1 records the layer-0 aggregate launches; later steps record exactly the cached ones fewer (four at the
    headline's layout) and the same other kernels, in the same order."""
    cfg, cached = _cfg(size)
    _, on, _ = _run(cfg, True, steps=3)
    _, off, _ = _run(cfg, False, steps=3)
    assert on[0] == off[0]
    for i in (1, 2):
        a_on, o_on = _split(on[i])
        a_off, o_off = _split(off[i])
        assert o_on == o_off, i
        assert len(a_on) == len(a_off) - cached, (i, len(a_on), len(a_off))
        assert a_off == _split(off[0])[0]


def _edit_features(g):
    g.x["node"].mul_(2)


def _edit_edges(g):
    e = g.edge_index[REL_PL]
    e[0, 0] = (e[0, 0] + 1) % g.x["path"].shape[0]


def _edit_raw(g):
    """A write torch's version counter of the feature tensor does not see (a second tensor over the same storage),
    followed by the call the contract asks for."""
    x = g.x["node"]
    v = x._version
    alias = torch.empty(0, dtype=x.dtype, device=x.device).set_(x.untyped_storage(), x.storage_offset(), x.shape,
                                                                 x.stride())
    alias.mul_(2)
    assert x._version == v
    g.features_changed()
    assert x._version > v and not ops.static_cache(x)


@pytest.mark.parametrize("edit", [_edit_features, _edit_edges, _edit_raw], ids=["mul_", "edge_index", "features_changed"])
@pytest.mark.parametrize("size", ["a", "b"])
def test_invalidation(size, edit):
    """An in-place torch edit of a feature tensor, of an edge_index, and features_changed() after a raw write, each
    between steps 2 and 3: step 3 aggregates again, and the trajectory equals the switch-off run's bitwise."""
    cfg, cached = _cfg(size)
    between = lambda i, g: edit(g) if i == 1 else None  # noqa: E731
    on, tr_on, _ = _run(cfg, True, between=between)
    off, tr_off, _ = _run(cfg, False, between=between)
    for i, (a, b) in enumerate(zip(on, off)):
        _same(a, b, f"step {i}")
    n = [len(_split(t)[0]) for t in tr_on]
    full = len(_split(tr_off[0])[0])
    # the edited tensor (or the relation's graph) feeds one cached launch: node -> link, or path -> link at (b);
    # (a) slices the path features inside the model, so its path -> link launch was never cached;
    # features_changed() speaks for every feature tensor of the graph
    redo = cached if edit is _edit_raw else 0 if (edit is _edit_edges and size == "a") else 1
    assert n == [full, full - cached, full - cached + redo, full - cached], n


@pytest.mark.parametrize("size", ["a", "b"])
def test_requires_grad_features_not_cached(size):
    """Features that require a gradient are aggregated every step; their gradient equals the switch-off run's."""
    cfg, _ = _cfg(size)

    def prepare(g):
        for t in g.x.values():
            t.requires_grad_(True)

    grads = []

    def between(i, g):
        grads.append([t.grad.clone() for t in g.x.values()])
        for t in g.x.values():
            t.grad = None

    on, tr_on, g = _run(cfg, True, steps=3, prepare=prepare, between=between)
    g_on, grads[:] = list(grads), []
    off, tr_off, _ = _run(cfg, False, steps=3, prepare=prepare, between=between)
    assert tr_on == tr_off and _split(tr_on[2])[0] == _split(tr_on[0])[0]
    assert not any(ops.static_cache(t) for t in g.x.values())
    for a, b in zip(on, off):
        _same(a, b)
    for a, b in zip(g_on, grads):
        _same(a, b)


def test_model_tensors_not_cached():
    """A concat GINConv above the first layer under no_grad takes the data-input branch (nothing needs a gradient),
    but its inputs were made inside the model: aggregated on every call, nothing stored on them."""
    cfg, _ = _cfg("b")
    g = synthetic_graph(cfg, seed=0, device=DEV)
    torch.manual_seed(3)
    layer = conv.GINLayer(2 * cfg.f_path, cfg.hidden, concat=True).to(DEV)
    x = g.x_dict()
    e = g.edge_index[REL_PL]
    with torch.no_grad():
        h_src, h_dst = x["path"] * 0.5, x["link"] * 0.5
        outs, counts = [], []
        for _ in range(3):
            with _lib.trace_launches() as tr:
                outs.append(layer((h_src, h_dst), e))
            counts.append(len(_split(tr.kernels)[0]))
        # the graph's own tensors through the same layer: cached from the second call on
        for _ in range(2):
            with _lib.trace_launches() as tr:
                layer((x["path"], x["link"]), e)
            counts.append(len(_split(tr.kernels)[0]))
    assert counts == [1, 1, 1, 1, 0], counts
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert not ops.static_cache(h_src) and not ops.is_static(h_src)
    assert len(ops.static_cache(x["path"])) == 1


@pytest.mark.parametrize("size", ["a", "b"])
def test_evaluation(size):
    """Two no_grad forwards: bitwise equal outputs, the second without the cached launches."""
    cfg, cached = _cfg(size)
    g = synthetic_graph(cfg, seed=0, device=DEV)
    model = _model(cfg).eval()
    outs, n = [], []
    with torch.no_grad():
        for _ in range(2):
            with _lib.trace_launches() as tr:
                outs.append(model(g.x_dict(), g.edge_index_dict(), g.batch["path"]))
            n.append(len(_split(tr.kernels)[0]))
    assert torch.equal(outs[0], outs[1])
    assert n[1] == n[0] - cached, n


def _store(n):
    from hgin.store import GraphStore
    cfg = CONFIGS["cfg1"]
    return GraphStore.build([synthetic_graph(cfg, seed=50 + i) for i in range(n)], device=DEV), cfg


def _clean(batch, handed_out=True):
    """No entry and no mark on a refilled buffer; where x_dict() handed it to a model, it is flagged volatile."""
    for t in batch.x.values():
        assert not ops.is_static(t) and not ops.static_cache(t)
        if handed_out:
            assert getattr(t, "_hgin_static", None) is False


@pytest.mark.parametrize("bs", [1, 2])
def test_refilled_buffers_captured_train(bs):
    """CapturedTrainStep over two different batches in turn (equal-sized graphs: the padded batch has no padding)
    equals eager exact-batch steps on store.collate(ids) bitwise; the refilled buffers never carry an entry or the
    mark."""
    from hgin.graphs import CapturedTrainStep
    store, cfg = _store(4)
    seq = [[0], [1], [0], [1]] if bs == 1 else [[0, 1], [2, 3], [1, 0], [3, 2]]
    m1 = _model(cfg)
    step = CapturedTrainStep(m1, torch.optim.Adam(m1.parameters(), lr=1e-3, capturable=True), store, batch_size=bs,
                             warmup_ids=seq[:1], warmup=1)
    cap = [step.step(ids).clone() for ids in seq[1:]]
    m2 = _model(cfg)
    o2 = torch.optim.Adam(m2.parameters(), lr=1e-3, capturable=True)
    eager = [train_step(m2, o2, store.collate(ids)).clone() for ids in seq][1:]
    torch.cuda.synchronize()
    _same(cap, eager, "loss")
    _same(_snap(m1, cap[-1]), _snap(m2, eager[-1]), "parameters / gradients")
    _clean(step.batch)


@pytest.mark.parametrize("bs", [1, 2])
def test_refilled_buffers_captured_eval(bs):
    from hgin.graphs import CapturedEvalStep
    store, cfg = _store(4)
    seq = [[0], [1], [0]] if bs == 1 else [[0, 1], [2, 3], [1, 0]]
    model = _model(cfg).eval()
    ev = CapturedEvalStep(model, store, batch_size=bs, warmup_ids=seq[:1], warmup=1)
    for ids in seq:
        loss = ev.step(ids).clone()
        b = store.collate(ids)
        out = ev.out[:b.y.numel()].clone()
        with torch.no_grad():
            want, want_loss = model.forward_loss(b.x_dict(), b.edge_index_dict(), b.batch["path"], b.y)
        assert torch.equal(loss, want_loss) and torch.equal(out, want), ids
    _clean(ev.batch)


@pytest.mark.parametrize("bs", [1, 2])
def test_refilled_buffers_small_batch_step(bs):
    """The fused small-batch step reads the refilled buffers itself (its own kernels, another summation order than the
    general path: against the eager exact-batch step it holds this suite's bound for that pair, loss 1e-5 relative and
    gradients 1e-4 of their norm, tests/smallbatch_cases.py); switch on and off are bitwise equal, each batch's result
    is its own, and the buffers stay unmarked."""
    from hgin.smallbatch import SmallBatchStep
    store, cfg = _store(4)
    seq = [[0], [1], [0]] if bs == 1 else [[0, 1], [2, 3], [1, 0]]
    runs = []
    for on in (True, False):
        was = ops.STATIC_AGG
        ops.STATIC_AGG = on
        try:
            m = _model(cfg)
            step = SmallBatchStep(m, torch.optim.Adam(m.parameters(), lr=0.0), store, batch_size=bs,
                                  warmup_ids=seq[:1], warmup=1)
            res = []
            for ids in seq:
                lv = step.step(ids).clone()
                res.append([lv] + [None if p.grad is None else p.grad.detach().clone() for p in m.parameters()])
            torch.cuda.synchronize()
            _clean(step.batch, handed_out=False)      # the fused kernels read the buffers by pointer
            runs.append(res)
        finally:
            ops.STATIC_AGG = was
    for a, b in zip(*runs):
        _same(a, b)
    m2 = _model(cfg)
    for ids, got in zip(seq, runs[0]):
        b = store.collate(ids)
        for p in m2.parameters():
            p.grad = None
        _, lv = m2.forward_loss(b.x_dict(), b.edge_index_dict(), b.batch["path"], b.y)
        torch.sqrt(lv).backward()
        print("small-batch vs eager", ids, float(got[0]), float(lv))
        assert abs(float(got[0]) - float(lv)) <= 1e-5 * abs(float(lv)), ids
        for (n, p), gg in zip(m2.named_parameters(), got[1:]):
            assert (p.grad is None) == (gg is None), n
            if gg is not None:
                d = float((gg.double() - p.grad.double()).norm())
                assert d <= 1e-4 * float(p.grad.double().norm()) + 1e-9, (ids, n, d)
    assert float(runs[0][0][0]) != float(runs[0][1][0])      # two different batches


@pytest.mark.parametrize("feat", ["f32", "bf16"])
def test_captured_static_step(feat):
    """Three CapturedStaticStep replays equal eager steps bitwise with the cache on; the cached tensors are the ones
    filled before the capture, at the same addresses after the replays."""
    from hgin.graphs import CapturedStaticStep
    cfg, cached = _cfg("b", feat)
    eager, _, _ = _run(cfg, True, steps=6, capturable=True)
    g = synthetic_graph(cfg, seed=0, device=DEV)
    model = _model(cfg)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, capturable=True)
    train_step(model, opt, g)
    before = {t: [(id(gr), c.data_ptr()) for gr, c in ops.static_cache(x)] for t, x in g.x.items()}
    assert sum(len(v) for v in before.values()) == cached
    st = CapturedStaticStep(model, opt, g, warmup=2)
    for i in range(3):
        loss = st.step()
        torch.cuda.synchronize()
        _same(_snap(model, loss), eager[3 + i], f"replay {i}")
    after = {t: [(id(gr), c.data_ptr()) for gr, c in ops.static_cache(x)] for t, x in g.x.items()}
    assert after == before


def test_captured_static_step_one_warmup_and_edit():
    """warmup=1 on a fresh graph (the capture's first lookup follows a single fill on the side stream) is correct;
    an in-place edit of the features between replays is followed (the step is captured again)."""
    from hgin.graphs import CapturedStaticStep
    cfg, _ = _cfg("b")
    between = lambda i, g: _edit_features(g) if i == 2 else None  # noqa: E731
    eager, _, _ = _run(cfg, False, steps=5, capturable=True, between=between)
    g = synthetic_graph(cfg, seed=0, device=DEV)
    model = _model(cfg)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, capturable=True)
    st = CapturedStaticStep(model, opt, g, warmup=1)
    for i in range(1, 5):
        loss = st.step()
        torch.cuda.synchronize()
        _same(_snap(model, loss), eager[i], f"replay {i}")
        between(i, g)


@pytest.mark.parametrize("feat", ["f32", "bf16"])
@pytest.mark.parametrize("size", ["a", "b"])
def test_cached_tensors_read_only(size, feat):
    """After three steps every cached tensor is bitwise a fresh aggregate of the same inputs."""
    cfg, cached = _cfg(size, feat)
    _, _, g = _run(cfg, True, steps=3)
    seen = 0
    for x in g.x.values():
        for graph, comb in ops.static_cache(x):
            fresh = ops.aggregate_into(graph.csr, x, None, None, ops.COMBINE_NONE, torch.empty_like(comb))
            assert torch.equal(comb, fresh)
            seen += 1
    assert seen == cached


def test_lifetime():
    """The entries die with the feature tensors: after the graph is dropped, the allocated bytes are back to what
    they were before it was built (model, optimizer state and gradients kept)."""
    cfg, cached = _cfg("b")
    model = _model(cfg)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)

    def steps():
        g = synthetic_graph(cfg, seed=0, device=DEV)
        for _ in range(2):
            train_step(model, opt, g)
        assert sum(len(ops.static_cache(t)) for t in g.x.values()) == cached
        del g

    def settled():
        torch.cuda.synchronize()
        gc.collect()
        torch.cuda.empty_cache()
        return torch.cuda.memory_allocated()

    steps()                 # optimizer state, gradients, lazily created constants
    base = settled()
    steps()
    assert settled() == base


def test_streams():
    """Fill on a side stream kept busy ahead of it; the first hit comes from the default stream with no device
    synchronize in between and must wait for the fill."""
    cfg, _ = _cfg("b")
    g = synthetic_graph(cfg, seed=0, device=DEV)
    x = g.x_dict()["path"]
    graph = ops.relation_graph(g.edge_index[REL_PL], x.shape[0], g.x["link"].shape[0])
    want = ops.aggregate_into(graph.csr, x, None, None, ops.COMBINE_NONE,
                              torch.empty(graph.n_dst, x.shape[1], device=DEV))
    busy = torch.randn(2048, 2048, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(20):
            busy = busy @ busy * 1e-3
        filled = ops._data_aggregate(graph, x)
    hit = ops._data_aggregate(graph, x)          # default stream, no synchronize
    got = hit.clone()
    torch.cuda.synchronize()
    assert hit is filled and torch.equal(got, want)

    # a whole step filled on a side stream, the next one on the default stream: the switch-off trajectory
    off, tr_off, _ = _run(cfg, False, steps=2)
    g = synthetic_graph(cfg, seed=0, device=DEV)
    model = _model(cfg)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        l0 = train_step(model, opt, g)
        s0 = _snap(model, l0)
    torch.cuda.current_stream().wait_stream(side)
    with _lib.trace_launches() as tr:
        l1 = train_step(model, opt, g)
    s1 = _snap(model, l1)
    torch.cuda.synchronize()
    _same(s0, off[0])
    _same(s1, off[1])
    assert len(_split(tr.kernels)[0]) == len(_split(tr_off[1])[0]) - 4      # the four cached launches are gone
