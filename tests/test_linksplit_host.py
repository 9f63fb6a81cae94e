"""Leakage-free edge splits (include/hgin.h A21), host side: the numpy restatement of the split rule on the C oracle's
Philox (``ref_parts``, which tests/test_gpu_linksplit.py pins the kernels to bit for bit), the properties the rule is
chosen for, the binomial part sizes, ABI 16 and the argument checks, all without a device."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

from oracle import c_oracle

TWO32 = 1 << 32
NEW_SYMBOLS = ("hgin_link_split_parts", "hgin_link_split_select_workspace_size", "hgin_link_split_select",
               "hgin_link_split_geometry")


def ref_bounds(val, test, disjoint=0.0):
    """(b_test, b_val, b_sup) as the header states them."""
    return (int(math.floor(test * TWO32)), int(math.floor((test + val) * TWO32)), int(math.floor(disjoint * TWO32)))


@functools.lru_cache(maxsize=1 << 20)
def _words(s, d, seed):
    """(x.x, x.y) of philox4x32_10(counter = {lo32(s), lo32(d), 1, 0}, key = {lo32(seed), hi32(seed)})."""
    seed &= (1 << 64) - 1
    x = c_oracle.philox4x32_10([s & 0xFFFFFFFF, d & 0xFFFFFFFF, 1, 0], [seed & 0xFFFFFFFF, seed >> 32])
    return int(x[0]), int(x[1])


def ref_parts(edge_index, seed, bounds, swap=False):
    """uint8 [E]: the part of every edge of an int64 [2, E] edge index (tensor or array).  ``swap`` reads the edges as
    (d, s), as the reverse relation is read."""
    ei = np.asarray(edge_index.cpu().numpy() if isinstance(edge_index, torch.Tensor) else edge_index, dtype=np.int64)
    src, dst = (ei[1], ei[0]) if swap else (ei[0], ei[1])
    w = np.array([_words(int(s), int(d), int(seed)) for s, d in zip(src, dst)], dtype=np.uint64).reshape(-1, 2)
    b_test, b_val, b_sup = (np.uint64(b) for b in bounds)
    part = np.zeros(len(src), dtype=np.uint8)
    part[w[:, 1] < b_sup] = 1
    part[w[:, 0] < b_val] = 2
    part[w[:, 0] < b_test] = 3
    return part


def _edges(E, n_src=97, n_dst=53, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(0, n_src, (E,), generator=g), torch.randint(0, n_dst, (E,), generator=g)])


def test_counter_word_two_keeps_the_stream_apart_from_the_samplers():
    """The samplers' counters have words 2 and 3 zero; the split's word 2 is 1, so (0, 0) is not Random123's
    known-answer block of the all-zero counter."""
    zero = [int(v) for v in c_oracle.philox4x32_10([0, 0, 0, 0], [0, 0])]
    assert zero == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert _words(0, 0, 0) != (zero[0], zero[1])


def test_a_pair_and_its_flipped_twin_share_a_part():
    ei = _edges(600)
    for fr in ((0.1, 0.2, 0.0), (0.1, 0.2, 0.3)):
        b = ref_bounds(*fr)
        for seed in (0, 2**40 + 3):
            fwd = ref_parts(ei, seed, b)
            assert np.array_equal(fwd, ref_parts(ei.flip(0), seed, b, swap=True))
            assert set(fwd.tolist()) == ({0, 2, 3} if fr[2] == 0 else {0, 1, 2, 3})
    assert not np.array_equal(ref_parts(ei, 0, ref_bounds(0.1, 0.2)), ref_parts(ei, 1, ref_bounds(0.1, 0.2)))


def test_duplicates_share_a_part_and_order_does_not_matter():
    ei = _edges(500, n_src=20, n_dst=15)
    pairs = (ei[0] * 15 + ei[1]).numpy()
    assert len(np.unique(pairs)) < len(pairs)
    part = ref_parts(ei, 7, ref_bounds(0.2, 0.2, 0.3))
    for p in np.unique(pairs):
        assert len(set(part[pairs == p].tolist())) == 1
    perm = torch.randperm(500, generator=torch.Generator().manual_seed(1))
    assert np.array_equal(ref_parts(ei[:, perm], 7, ref_bounds(0.2, 0.2, 0.3)), part[perm.numpy()])


def test_degenerate_fractions():
    ei = _edges(300)
    assert ref_bounds(0.0, 1.0) == (TWO32, TWO32, 0)
    assert (ref_parts(ei, 3, ref_bounds(0.0, 1.0)) == 3).all()
    assert (ref_parts(ei, 3, ref_bounds(1.0, 0.0)) == 2).all()
    assert (ref_parts(ei, 3, ref_bounds(0.0, 0.0, 0.0)) == 0).all()
    assert (ref_parts(ei, 3, ref_bounds(0.0, 0.0, 1.0)) == 1).all()
    assert not (ref_parts(ei, 3, ref_bounds(0.1, 0.2, 1.0)) == 0).any()


def test_part_sizes_are_binomial():
    """20,000 distinct pairs, (val, test) = (0.1, 0.2): every part count within 5 sqrt(E p (1 - p)) of E p — the
    binomial's own spread (a 5-sigma bound), not a measurement."""
    E = 20_000
    ids = torch.randperm(400 * 300, generator=torch.Generator().manual_seed(11))[:E]
    ei = torch.stack([ids // 300, ids % 300])
    assert len(np.unique((ei[0] * 300 + ei[1]).numpy())) == E
    for disjoint in (0.0, 0.25):
        part = ref_parts(ei, 2024, ref_bounds(0.1, 0.2, disjoint))
        want = {3: 0.2, 2: 0.1, 1: 0.7 * disjoint, 0: 0.7 * (1.0 - disjoint)}
        for p, prob in want.items():
            n = int((part == p).sum())
            assert abs(n - E * prob) <= 5.0 * math.sqrt(E * prob * (1.0 - prob)), (disjoint, p, n, E * prob)


def test_abi_16_and_the_header_section():
    from conftest import ROOT
    from hgin import _lib
    assert _lib.ABI_VERSION == 16
    assert _lib.lib().hgin_abi_version() == 16
    text = open(os.path.join(ROOT, "include", "hgin.h")).read()
    assert int(re.search(r"#define HGIN_ABI_VERSION (\d+)", text).group(1)) == 16
    a21 = text[text.index("---- A21"):]
    a21 = a21[:a21.index("---- F4")]
    for name in NEW_SYMBOLS:
        assert name in _lib.exported_symbols() and hasattr(_lib.lib(), name), name
        assert re.search(r"\bint " + name + r"\(", a21), name
    for word in ("(uint32)s, (uint32)d, 1, 0", "swap = 1", "b_test = floor(test * 2^32)", "floor((test + val) * 2^32)",
                 "floor(disjoint * 2^32)", "flipped twin", "multi-edge", "does not depend on edge order", "binomial",
                 "three plain launches", "No workgroup waits on another", "out_eid"):
        assert word in a21, word


def test_python_surface():
    import inspect

    import hgin
    from hgin import linksplit, train
    for name in ("link_split", "link_split_parts", "link_split_select", "LinkSplit"):
        assert name in hgin.__all__ and hasattr(hgin, name), name
    sig = inspect.signature(train.link_train_step)
    assert list(sig.parameters) == ["model", "opt", "graph", "predictor", "step", "pos", "known"]
    assert sig.parameters["pos"].default is None and sig.parameters["known"].default is None
    sig = inspect.signature(linksplit.link_split)
    assert [(n, p.default) for n, p in sig.parameters.items()][2:] == [
        ("rev_relation", "auto"), ("val", 0.1), ("test", 0.1), ("disjoint", 0.0), ("seed", 0)]
    fields = {f.name for f in linksplit.LinkSplit.__dataclass_fields__.values()}
    assert {"train_graph", "val_graph", "test_graph", "train_pos", "val_pos", "test_pos", "known", "counts"} <= fields
    assert linksplit.split_bounds(0.1, 0.2, 0.3) == ref_bounds(0.1, 0.2, 0.3)
    assert linksplit.split_bounds(0.0, 1.0) == (TWO32, TWO32, 0)


def test_geometry_is_exposed_and_small_enough_to_test_past_one_scan_pass():
    from hgin import linksplit
    tile, width = linksplit.split_geometry()
    assert tile >= 64 and tile % 64 == 0 and width >= 1
    assert tile * width + 1 <= 8 * 1024 * 1024 + 1


# ---------------------------------------------------------------------------------------------------
# validation: before any device is needed
# ---------------------------------------------------------------------------------------------------
def _graph():
    from hgin.data import CONFIGS, synthetic_graph
    return synthetic_graph(CONFIGS["cfg1"], seed=0)


def test_fraction_errors_on_cpu_tensors():
    import hgin
    from hgin.data import REL_PL
    ei, g = _edges(10), _graph()
    for kw in (dict(val=-0.1, test=0.1), dict(val=0.1, test=1.5), dict(val=0.6, test=0.5),
               dict(val=0.1, test=0.1, disjoint=1.01), dict(val=float("nan"), test=0.1)):
        with pytest.raises(ValueError):
            hgin.link_split_parts(ei, 0, **kw)
        with pytest.raises(ValueError):
            hgin.link_split(g, REL_PL, **kw)
    for kw in (dict(val="0.1", test=0.1), dict(val=0.1, test=None), dict(val=0.1, test=0.1, disjoint=True)):
        with pytest.raises(TypeError):
            hgin.link_split_parts(ei, 0, **kw)
        with pytest.raises(TypeError):
            hgin.link_split(g, REL_PL, **kw)
    with pytest.raises(TypeError):
        hgin.link_split_parts(ei, 0.5, 0.1, 0.1)


def test_edge_index_errors_on_cpu_tensors():
    import hgin
    from hgin.data import REL_PL, HeteroGraph
    with pytest.raises(TypeError):
        hgin.link_split_parts(_edges(10).to(torch.int32), 0, 0.1, 0.1)
    with pytest.raises(TypeError):
        hgin.link_split_parts([[0, 1], [1, 0]], 0, 0.1, 0.1)
    with pytest.raises(ValueError):
        hgin.link_split_parts(_edges(10).t().contiguous(), 0, 0.1, 0.1)
    with pytest.raises(ValueError):
        hgin.link_split_parts(torch.zeros(10, dtype=torch.int64), 0, 0.1, 0.1)
    part = torch.zeros(10, dtype=torch.uint8)
    with pytest.raises(TypeError):
        hgin.link_split_select(_edges(10).to(torch.int32), part, (0,))
    with pytest.raises(TypeError):
        hgin.link_split_select(_edges(10), part.to(torch.int64), (0,))
    with pytest.raises(ValueError):
        hgin.link_split_select(_edges(10), part[:9], (0,))
    with pytest.raises(ValueError):
        hgin.link_split_select(_edges(10), part, (0, 4))
    with pytest.raises(TypeError):
        hgin.link_split_select(_edges(10), part, (0.0,))
    g = _graph()
    bad = HeteroGraph(g.x, dict(g.edge_index), g.y, g.batch)
    bad.edge_index[REL_PL] = g.edge_index[REL_PL].to(torch.int32)
    with pytest.raises(TypeError):
        hgin.link_split(bad, REL_PL)


def test_relation_errors_and_the_auto_reverse():
    import hgin
    from hgin import linksplit
    from hgin.data import REL_LN, REL_LP, REL_NL, REL_PL, HeteroGraph
    g = _graph()
    with pytest.raises(ValueError, match="no relation"):
        hgin.link_split(g, ("path", "likes", "link"))
    with pytest.raises(ValueError, match="no relation"):
        hgin.link_split(g, REL_PL, rev_relation=("link", "likes", "path"))
    with pytest.raises(ValueError, match="does not run"):
        hgin.link_split(g, REL_PL, rev_relation=REL_LN)
    with pytest.raises(ValueError):
        hgin.link_split(g, REL_PL, rev_relation="reverse")
    assert linksplit._reverse_of("t", g, REL_PL, "auto") == REL_LP
    assert linksplit._reverse_of("t", g, REL_LN, "auto") == REL_NL
    assert linksplit._reverse_of("t", g, REL_PL, None) is None
    two = HeteroGraph(g.x, dict(g.edge_index), g.y, g.batch)
    two.edge_index[("link", "carries", "path")] = g.edge_index[REL_LP]
    with pytest.raises(ValueError, match="several relations"):
        hgin.link_split(two, REL_PL)
    assert linksplit._reverse_of("t", two, REL_PL, REL_LP) == REL_LP
    none = HeteroGraph(g.x, {REL_PL: g.edge_index[REL_PL]}, g.y, g.batch)
    assert linksplit._reverse_of("t", none, REL_PL, "auto") is None


def test_a_padded_batch_is_refused():
    import hgin
    from hgin.data import REL_PL
    from hgin.store import PaddedBatch
    pb = object.__new__(PaddedBatch)
    with pytest.raises(ValueError, match="PaddedBatch"):
        hgin.link_split(pb, REL_PL)


def test_valid_arguments_on_cpu_tensors_name_the_missing_device():
    import hgin
    from hgin.data import REL_PL
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hgin.link_split_parts(_edges(10), 0, 0.1, 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hgin.link_split(_graph(), REL_PL)


# ---------------------------------------------------------------------------------------------------
# C argument checks: HGIN_E_ARG / HGIN_E_WORKSPACE before any launch
# ---------------------------------------------------------------------------------------------------
_Q = ctypes.c_void_p(256)


def test_c_argument_errors_do_not_touch_the_device():
    from hgin import _lib
    lib = _lib.lib()
    err = lib.hgin_last_error

    def parts(ei=_Q, E=4, swap=0, bt=1, bv=2, bs=0, part=_Q, hist=_Q):
        return lib.hgin_link_split_parts(ei, E, swap, 0, bt, bv, bs, part, hist, None)

    assert parts(E=-1) == -1 and b"E = -1" in err()
    assert parts(E=1 << 40) == -1 and b"2^40" in err()
    assert parts(swap=2) == -1 and b"swap" in err()
    assert parts(bv=TWO32 + 1) == -1 and b"above 2^32" in err()
    assert parts(bs=TWO32 + 1) == -1 and b"above 2^32" in err()
    assert parts(bt=3, bv=2) == -1 and b"b_val < b_test" in err()
    assert parts(ei=None) == -1 and b"edge_index NULL" in err()
    assert parts(part=None) == -1 and b"part NULL" in err()
    assert parts(hist=None) == -1 and b"hist NULL" in err()
    assert parts(E=0, ei=None, part=None, hist=None) == 0          # nothing to do, nothing dereferenced

    size = ctypes.c_size_t(0)
    assert lib.hgin_link_split_select_workspace_size(10, None) == -1
    assert lib.hgin_link_split_select_workspace_size(-1, ctypes.byref(size)) == -1
    tile, width = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.hgin_link_split_geometry(ctypes.byref(tile), ctypes.byref(width)) == 0
    assert lib.hgin_link_split_geometry(None, None) == 0
    n_tiles = 5
    assert lib.hgin_link_split_select_workspace_size(n_tiles * tile.value, ctypes.byref(size)) == 0
    assert size.value == 256 + 256 and size.value >= 4 * n_tiles + 8 * (n_tiles + 1)

    def select(ei=_Q, part=_Q, E=4, mask=1, out=_Q, eid=_Q, n_out=2, ws=_Q, ws_bytes=1 << 20):
        return lib.hgin_link_split_select(ei, part, E, mask, out, eid, n_out, ws, ws_bytes, None)

    assert select(E=-1) == -1 and b"E = -1" in err()
    assert select(mask=16) == -1 and b"keep_mask = 16" in err()
    assert select(mask=-1) == -1 and b"keep_mask" in err()
    assert select(n_out=5) == -1 and b"n_out = 5" in err()
    assert select(n_out=-1) == -1 and b"n_out" in err()
    assert select(part=None) == -1 and b"part NULL" in err()
    assert select(ei=None) == -1 and b"edge_index NULL" in err()
    assert select(out=None) == -1 and b"out_edge NULL" in err()
    assert select(eid=None) == -1 and b"out_eid NULL" in err()
    assert select(ws=None) == -3 and b"workspace" in err()
    assert select(ws_bytes=8) == -3 and b"workspace" in err()
    assert select(E=0, n_out=0, ei=None, part=None, out=None, eid=None, ws=None, ws_bytes=0) == 0
    assert select(E=0, n_out=1) == -1
