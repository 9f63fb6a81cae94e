"""The link-prediction training path on the GPU (include/hgin.h A13 / A14, hgin/linkpred.py, hgin/train.py).

Negatives: bit for bit the C oracle's sampler.  Loss and gradients: against this suite's float64 CPU reference
(tests/test_linkpred_host.py) built from the oracle's negatives, and against the unfused ``link_loss`` on the GPU:
|d loss| <= 1e-5 |loss|, ||d g|| <= 1e-5 ||g_ref|| + 1e-9 (the project's embedding tolerance; an fp32 evaluation of
the same expression at these shapes is within 4e-7 of float64, so a dropped or doubled term shows).  Determinism:
bitwise.  Ranks: exact on integer-valued embeddings.  Model level: ``encode`` and five ``link_train_step``s against
the CPU replica (oracle convs + the float64 loss + the oracle's negatives + torch's Adam)."""
import functools

import numpy as np
import pytest
import torch

from test_linkpred_host import ref_loss, ref_loss_and_grads, ref_metrics, ref_ranks

DEV = "cuda"
pytestmark = pytest.mark.gpu

N_SRC, E, SEED = 37, 211, 0x1234ABCD5678
REL_PL = ("path", "uses", "link")

# the issue's grid, plus the widths at which the forward leaves the row-in-registers form for the looped one
# (more than 64 pieces per row: F = 260 on the float4 path, F = 70 on the scalar path)
GRID = [(n_dst, k, off, F) for n_dst in (1, 5, 53) for k in (1, 3, 5) for off in (0, 6, 2**32 + 1)
        for F in (6, 8, 128, 256)]
# and a destination table wide enough that many rows are neither a positive's destination nor ever drawn
EXTRA = [(53, 3, 6, 260), (5, 5, 2**32 + 1, 70), (53, 1, 0, 512), (401, 1, 6, 8)]
CASES = GRID + EXTRA


def _inputs(n_dst, F, integer=False):
    g = torch.Generator().manual_seed(1000 * n_dst + F)
    # sources from 30 of the 37 rows: rows 30..36 (and whatever the draw misses) have no positive
    # destinations from the first four fifths of the table: the rest is reached by drawn negatives only
    pos = torch.stack([torch.randint(0, 30, (E,), generator=g),
                       torch.randint(0, n_dst - n_dst // 5, (E,), generator=g)])
    if integer:
        zs = torch.randint(-2, 3, (N_SRC, F), generator=g).float()
        zd = torch.randint(-2, 3, (n_dst, F), generator=g).float()
    else:
        zs = torch.randn(N_SRC, F, generator=g) * 0.5
        zd = torch.randn(n_dst, F, generator=g) * 0.5
    return pos, zs, zd


def _run_fused(zs, zd, pos, k, off):
    """(loss, g_src, g_dst, negatives) of one fused forward + backward on the device."""
    from hgin.linkpred import _SampledLinkLossFn, sampled_link_loss
    a, b = zs.detach().clone().requires_grad_(True), zd.detach().clone().requires_grad_(True)
    loss = sampled_link_loss(a, b, pos, k, SEED, off)
    assert isinstance(loss.grad_fn, _SampledLinkLossFn._backward_cls)
    coef, neg, sa, sb = loss.grad_fn.saved_tensors   # nothing else is saved
    assert tuple(coef.shape) == (pos.size(1) * (1 + k),) and sa.data_ptr() == a.data_ptr() and sb.data_ptr() == b.data_ptr()
    loss.backward()
    return loss.detach(), a.grad, b.grad, neg


@functools.lru_cache(maxsize=None)
def _case(n_dst, k, off, F):
    from oracle import c_oracle
    pos, zs, zd = _inputs(n_dst, F)
    posd, zsd, zdd = pos.to(DEV), zs.to(DEV), zd.to(DEV)
    loss, g_src, g_dst, neg = _run_fused(zsd, zdd, posd, k, off)
    want_neg = c_oracle.neg_sample(SEED, off, E * k, n_dst)
    ref = ref_loss_and_grads(zs, zd, pos, want_neg, k)
    return dict(pos=pos, posd=posd, zs=zs, zd=zd, zsd=zsd, zdd=zdd, loss=loss, g_src=g_src, g_dst=g_dst, neg=neg,
                want_neg=want_neg, ref=ref)


def _check(loss, g_src, g_dst, ref, what):
    rl, rs, rd = ref
    dl = abs(float(loss) - float(rl))
    ds = float((g_src.detach().cpu().double() - rs.double().cpu()).norm())
    dd = float((g_dst.detach().cpu().double() - rd.double().cpu()).norm())
    print(f"{what}: |dloss|/|loss| {dl / abs(float(rl)):.3g}  ||dg_src||/||g|| {ds / float(rs.double().norm()):.3g}  "
          f"||dg_dst||/||g|| {dd / float(rd.double().norm()):.3g}")
    assert dl <= 1e-5 * abs(float(rl)), (what, dl, float(rl))
    assert ds <= 1e-5 * float(rs.double().norm()) + 1e-9, (what, ds)
    assert dd <= 1e-5 * float(rd.double().norm()) + 1e-9, (what, dd)


@pytest.mark.parametrize("n_dst,k,off,F", CASES)
def test_negatives_are_the_oracle_samplers(n_dst, k, off, F):
    c = _case(n_dst, k, off, F)
    neg = c["neg"].cpu()
    assert neg.dtype == torch.int64 and tuple(neg.shape) == (2, E * k)
    assert np.array_equal(neg[1].numpy(), c["want_neg"].astype(np.int64))
    assert torch.equal(neg[0], c["pos"][0].repeat_interleave(k))
    # and they are the pairs the unfused path draws
    from hgin.linkpred import negative_edges
    assert torch.equal(negative_edges(c["posd"], n_dst, k, SEED, off).cpu(), neg)


@pytest.mark.parametrize("n_dst,k,off,F", CASES)
def test_loss_and_gradients_vs_float64_reference_and_link_loss(n_dst, k, off, F):
    from hgin.linkpred import link_loss
    c = _case(n_dst, k, off, F)
    assert c["loss"].dim() == 0 and c["loss"].dtype == torch.float32
    _check(c["loss"], c["g_src"], c["g_dst"], c["ref"], "fused vs float64")
    a, b = c["zsd"].clone().requires_grad_(True), c["zdd"].clone().requires_grad_(True)
    base = link_loss(a, b, c["posd"], k, SEED, off)
    base.backward()
    _check(c["loss"], c["g_src"], c["g_dst"], (base.detach().cpu(), a.grad.cpu(), b.grad.cpu()),
           "fused vs link_loss")


@pytest.mark.parametrize("n_dst,k,off,F", CASES)
def test_bitwise_determinism_and_exact_zero_rows(n_dst, k, off, F):
    c = _case(n_dst, k, off, F)
    loss, g_src, g_dst, neg = _run_fused(c["zsd"], c["zdd"], c["posd"], k, off)
    assert torch.equal(loss, c["loss"]) and torch.equal(g_src, c["g_src"]) and torch.equal(g_dst, c["g_dst"])
    assert torch.equal(neg, c["neg"])
    no_pos = torch.ones(N_SRC, dtype=torch.bool)
    no_pos[c["pos"][0]] = False
    assert int(no_pos.sum()) >= 7
    rows = c["g_src"].cpu()[no_pos]
    assert rows.numel() and bool((rows == 0).all()) and not bool(torch.signbit(rows).any())
    untouched = torch.ones(n_dst, dtype=torch.bool)
    untouched[c["pos"][1]] = False
    untouched[torch.as_tensor(c["want_neg"].astype(np.int64))] = False
    if n_dst == 401:
        assert int(untouched.sum()) >= 10   # destinations that are no positive's and are never drawn
    rows = c["g_dst"].cpu()[untouched]
    assert bool((rows == 0).all()) and not bool(torch.signbit(rows).any())


@pytest.mark.parametrize("F,k", [(8, 3), (70, 5), (128, 1)])
def test_non_contiguous_odd_stride_views(F, k):
    """Embeddings that are column windows of wider buffers (row stride odd, start not 16-byte aligned): the scalar
    path; the gradient reaches the window and nothing else."""
    from hgin.linkpred import sampled_link_loss
    from oracle import c_oracle
    n_dst, off = 53, 6
    pos, zs, zd = _inputs(n_dst, F)
    g = torch.Generator().manual_seed(5)
    bs = torch.randn(N_SRC, 2 * F + 1, generator=g)
    bd = torch.randn(n_dst, F + 3, generator=g)
    bs[:, 1:F + 1], bd[:, 3:] = zs, zd
    bs, bd = bs.to(DEV).requires_grad_(True), bd.to(DEV).requires_grad_(True)
    vs, vd = bs[:, 1:F + 1], bd[:, 3:]
    assert not vs.is_contiguous() and vs.stride(0) % 2 == 1 and vd.stride(0) % 2 == 1
    loss = sampled_link_loss(vs, vd, pos.to(DEV), k, SEED, off)
    loss.backward()
    ref = ref_loss_and_grads(zs, zd, pos, c_oracle.neg_sample(SEED, off, E * k, n_dst), k)
    _check(loss.detach(), bs.grad[:, 1:F + 1], bd.grad[:, 3:], ref, "strided views vs float64")
    assert bool((bs.grad[:, 0] == 0).all()) and bool((bs.grad[:, F + 1:] == 0).all())
    assert bool((bd.grad[:, :3] == 0).all())


def test_upstream_gradient_scales_both_gradients():
    """g is read from device memory: d(3 loss) = 3 d(loss) bitwise up to the one extra rounding of g * c."""
    from hgin.linkpred import sampled_link_loss
    c = _case(53, 3, 6, 128)
    a, b = c["zsd"].clone().requires_grad_(True), c["zdd"].clone().requires_grad_(True)
    (sampled_link_loss(a, b, c["posd"], 3, SEED, 6) * 3.0).backward()
    _check(c["loss"], a.grad / 3.0, b.grad / 3.0, c["ref"], "3 x loss")


def test_launch_tags():
    from hgin import _lib
    c = _case(53, 3, 6, 128)
    with _lib.trace_launches() as tr:
        _run_fused(c["zsd"], c["zdd"], c["posd"], 3, 6)
    tags = tr.kernels
    assert "k_link_fwd<4,32,ONE,LOSS>" in tags and "k_link_loss_sum" in tags
    assert "k_link_bwd_src<4,32>" in tags and "k_link_bwd_dst<4,32>" in tags
    c = _case(53, 3, 6, 260)
    with _lib.trace_launches() as tr:
        _run_fused(c["zsd"], c["zdd"], c["posd"], 3, 6)
    assert "k_link_fwd<4,64,LOOP,LOSS>" in tr.kernels


def test_bad_arguments_raise_before_any_launch():
    from hgin import HginError
    from hgin.linkpred import link_ranks, sampled_link_loss
    c = _case(53, 3, 6, 128)
    with pytest.raises(TypeError, match="float32"):
        sampled_link_loss(c["zsd"].bfloat16(), c["zdd"].bfloat16(), c["posd"], 3, SEED)
    with pytest.raises(TypeError, match="float32"):
        link_ranks(c["zsd"].double(), c["zdd"].double(), c["posd"], 3, SEED)
    with pytest.raises(ValueError, match="k >= 1"):
        sampled_link_loss(c["zsd"], c["zdd"], c["posd"], 0, SEED)
    with pytest.raises(ValueError, match="E >= 1"):
        sampled_link_loss(c["zsd"], c["zdd"], c["posd"][:, :0], 3, SEED)
    with pytest.raises(IndexError):   # a destination id past z_dst: caught by the cached CSR build's range check
        sampled_link_loss(c["zsd"], c["zdd"][:20], c["posd"].clone(), 3, SEED)
    assert HginError is not None


# ---------------------------------------------------------------------------------------------------
# ranks / metrics
# ---------------------------------------------------------------------------------------------------
RANK_CASES = [(n_dst, k, off, F) for n_dst in (1, 5, 53) for k in (1, 3, 5) for off in (6, 2**32 + 1)
              for F in (6, 8, 64)]


@pytest.mark.parametrize("n_dst,k,off,F", RANK_CASES)
def test_ranks_exact_on_integer_embeddings_and_metrics(n_dst, k, off, F):
    """Embeddings in {-2..2}: every dot product is an exact fp32 integer in any summation order, so the counts are
    exact; at n_dst = 1 and 5 drawn negatives collide with the true destination and tie exactly."""
    from hgin.linkpred import link_metrics, link_ranks
    from oracle import c_oracle
    pos, zs, zd = _inputs(n_dst, F, integer=True)
    nd = c_oracle.neg_sample(SEED, off, E * k, n_dst).astype(np.int64)
    zsn, zdn = zs.numpy().astype(np.int64), zd.numpy().astype(np.int64)
    s_pos = (zsn[pos[0].numpy()] * zdn[pos[1].numpy()]).sum(1)
    s_neg = (zsn[pos[0].repeat_interleave(k).numpy()] * zdn[nd]).sum(1)
    want_gt, want_eq = ref_ranks(s_pos, s_neg, k)
    if n_dst <= 5:
        assert int(want_eq.sum()) > 0
    gt, eq = link_ranks(zs.to(DEV), zd.to(DEV), pos.to(DEV), k, SEED, off)
    assert gt.dtype == torch.int32 and eq.dtype == torch.int32
    assert np.array_equal(gt.cpu().numpy(), want_gt) and np.array_equal(eq.cpu().numpy(), want_eq)
    got = link_metrics(zs.to(DEV), zd.to(DEV), pos.to(DEV), k, SEED, off)
    want = ref_metrics(want_gt, want_eq, k)
    assert sorted(got) == sorted(want) == ["auc", "hits@1", "hits@10", "hits@3", "mrr"]
    for name, v in want.items():
        assert got[name].is_cuda and got[name].dim() == 0
        assert abs(float(got[name]) - v) <= 1e-6, (name, float(got[name]), v)


def test_rank_kernel_writes_nothing_else_and_tags():
    from hgin import _lib
    from hgin.linkpred import link_ranks
    pos, zs, zd = _inputs(53, 64, integer=True)
    with _lib.trace_launches() as tr:
        link_ranks(zs.to(DEV), zd.to(DEV), pos.to(DEV), 3, SEED)
    assert [t for t in tr.kernels if t.startswith("k_link")] == ["k_link_fwd<4,16,ONE,RANK>"]


# ---------------------------------------------------------------------------------------------------
# model level (cfg1 synthetic graph)
# ---------------------------------------------------------------------------------------------------
def _cfg1():
    from hgin.data import CONFIGS, synthetic_graph
    cfg = CONFIGS["cfg1"]
    return cfg, synthetic_graph(cfg, seed=0)


def _gin_pair():
    """(oracle model on the CPU, hgin.HetroGIN on the device) with one set of initial weights, 2 layers."""
    import hgin
    from oracle.pyg_cpu import OracleHetroGIN
    cfg, g = _cfg1()
    assert cfg.layers == 2 and not cfg.divided_features and not cfg.bl_features
    ic = lambda: {"link": cfg.f_link, "path": cfg.f_path, "node": cfg.f_node}  # noqa: E731
    torch.manual_seed(1997)
    ref = OracleHetroGIN(**cfg.model_kwargs(ic())).train()
    model = hgin.HetroGIN(**cfg.model_kwargs(ic()))
    model.load_state_dict(ref.state_dict())
    return cfg, g, ref, model.to(DEV).train()


def _oracle_encode(ref, x_dict, edge_index_dict):
    """The reference forward's slicing and conv loop (models.py:333-342, :355-359) without the read-out, on the
    oracle's own conv stack, layer by layer (cfg1 flags: neither divided nor baseline features)."""
    x = dict(x_dict)
    x["path"] = torch.cat([x["path"][:, 0:3], x["path"][:, 6].reshape(-1, 1)], axis=1)[:, 0:3]
    x["link"] = torch.cat([x["link"][:, 0:3], x["link"][:, 4:7]], axis=1)[:, 0:3]
    for i in range(ref.num_layers):
        x = ref.convs[i](x, edge_index_dict)
        for t in list(x.keys()):
            x[t] = torch.nn.functional.dropout(x[t], p=ref.dropout, training=ref.training)
    return x


def test_encode_vs_oracle_conv_stack():
    cfg, g, ref, model = _gin_pair()
    gd = g.to(DEV)
    xd = gd.x_dict()
    z = model.encode(xd, gd.edge_index_dict())
    assert all(xd[t] is gd.x[t] for t in xd)   # the caller's dict is left alone
    want = _oracle_encode(ref, g.x_dict(), g.edge_index_dict())
    assert sorted(z) == sorted(want) == ["link", "node", "path"]
    for t, w in want.items():
        assert tuple(z[t].shape) == (g.num_nodes(t), cfg.hidden)
        d = (z[t].detach().cpu() - w.detach()).abs()
        assert bool((d <= 1e-5 + 1e-5 * w.detach().abs()).all()), (t, float(d.max()))
    # forward still is read-out(encode)
    out = model(gd.x_dict(), gd.edge_index_dict(), gd.batch["path"])
    want_out = ref(g.x_dict(), g.edge_index_dict(), g.batch["path"])
    assert bool(((out.detach().cpu() - want_out.detach()).abs() <= 1e-5 + 1e-5 * want_out.detach().abs()).all())


def test_five_link_train_steps_follow_the_cpu_replica():
    import hgin
    from oracle import c_oracle
    cfg, g, ref, model = _gin_pair()
    gd = g.to(DEV)
    k, seed = 3, 7
    pos = g.edge_index[REL_PL]
    n_e = int(pos.size(1))
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    pred = hgin.LinkPredictor(model, REL_PL, k, seed)
    got = [hgin.link_train_step(model, opt, gd, pred, step=s) for s in range(5)]
    assert all(v.is_cuda and v.dim() == 0 and not v.requires_grad for v in got)
    got = [float(v) for v in got]

    ropt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    want = []
    for s in range(5):
        ropt.zero_grad()
        z = _oracle_encode(ref, g.x_dict(), g.edge_index_dict())
        nd = c_oracle.neg_sample(seed, s * n_e * k, n_e * k, cfg.n_link)
        loss = ref_loss(z["path"].double(), z["link"].double(), pos, nd, k)
        loss.backward()
        ropt.step()
        want.append(float(loss.detach()))
    print("link loss trajectory gpu", got, "cpu", want)
    for s, (a, b) in enumerate(zip(got, want)):
        assert abs(a - b) <= 1e-4 * abs(b), (s, a, b)
    assert got[4] < got[0]


def _fp32_scores_like_the_kernel(zs, zd, src, dst):
    """<zs[src], zd[dst]> in the fused forward's own fp32 order at F = 8 (two lanes of four elements: sequential
    multiply-add per lane, then the two lane sums added), so that host and device agree on every tie and order."""
    a, b = zs[src].astype(np.float32), zd[dst].astype(np.float32)
    assert a.shape[1] == 8
    lanes = []
    for lo in (0, 4):
        acc = np.zeros(a.shape[0], np.float32)
        for f in range(lo, lo + 4):
            acc = (acc + (a[:, f] * b[:, f]).astype(np.float32)).astype(np.float32)
        lanes.append(acc)
    return (lanes[0] + lanes[1]).astype(np.float32)


def test_predictor_metrics_equal_the_reference_on_the_gpu_embeddings():
    import hgin
    from oracle import c_oracle
    cfg, g, _, model = _gin_pair()
    gd = g.to(DEV)
    k, seed = 3, 7
    pred = hgin.LinkPredictor(model, REL_PL, k, seed)
    m = pred.metrics(gd)
    assert model.training   # the mode is restored
    assert all(not v.requires_grad for v in m.values())
    auc = float(m["auc"])
    assert 0.0 <= auc <= 1.0
    model.eval()
    with torch.no_grad():
        z = model.encode(gd.x_dict(), gd.edge_index_dict())
    zs, zd = z["path"].cpu().numpy(), z["link"].cpu().numpy()
    pos = g.edge_index[REL_PL].numpy()
    n_e = pos.shape[1]
    nd = c_oracle.neg_sample(seed, 0, n_e * k, cfg.n_link).astype(np.int64)
    s_pos = _fp32_scores_like_the_kernel(zs, zd, pos[0], pos[1])
    s_neg = _fp32_scores_like_the_kernel(zs, zd, np.repeat(pos[0], k), nd)
    want = ref_metrics(*ref_ranks(s_pos, s_neg, k), k)
    for name, v in want.items():
        assert abs(float(m[name]) - v) <= 1e-12, (name, float(m[name]), v)
    # an explicit subset of positives
    sub = gd.edge_index[REL_PL][:, :100].contiguous()
    m2 = pred.metrics(gd, pos=sub)
    nd2 = c_oracle.neg_sample(seed, 0, 100 * k, cfg.n_link).astype(np.int64)
    want2 = ref_metrics(*ref_ranks(s_pos[:100], _fp32_scores_like_the_kernel(zs, zd, np.repeat(pos[0, :100], k), nd2),
                                   k), k)
    assert abs(float(m2["auc"]) - want2["auc"]) <= 1e-12


def test_hetrogat_encode_width_and_one_link_train_step():
    """HetroGAT, heads 16 x 8, one layer: encode is [N_t, 128]; one link_train_step leaves a finite gradient on every
    parameter the link loss of ('path', 'uses', 'link') reaches — the GAT layers of the two relations that write
    the path and link embeddings (the read-out and the relations into 'node' are not part of this loss, and have
    no gradient at all) — and on no parameter a non-finite one."""
    import hgin
    cfg, g = _cfg1()
    gd = g.to(DEV)
    torch.manual_seed(1997)
    model = hgin.HetroGAT(input_channels={"link": cfg.f_link, "path": cfg.f_path, "node": cfg.f_node},
                          node_embedding_size=8, message_passing_layers=1, dropout=0.0, heads=16, concat_path=True,
                          bl_features=False, divided_features=False, global_feats=False, mlp_layers=[128, 32],
                          act="torch.nn.PReLU()", mlp_head_act=None, mlp_bn=False).to(DEV).train()
    assert hasattr(model, "encode")
    with torch.no_grad():
        z = model.encode(gd.x_dict(), gd.edge_index_dict())   # also materialises the lazy projections
    for t in ("path", "link", "node"):
        assert tuple(z[t].shape) == (g.num_nodes(t), 128) and z[t].dtype == torch.float32
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    pred = hgin.LinkPredictor(model, REL_PL, 3, 7)
    loss = hgin.link_train_step(model, opt, gd, pred, step=0)
    assert bool(torch.isfinite(loss))
    reached = 0
    for name, p in model.named_parameters():
        if name.startswith("convs.0.convs.path__uses__link.") or name.startswith("convs.0.convs.link__includes__path."):
            assert p.grad is not None, name
            reached += 1
        if p.grad is not None:
            assert bool(torch.isfinite(p.grad).all()), name
    assert reached >= 8
