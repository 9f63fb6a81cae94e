"""The exact three-plane oracles of tests/split_oracles.py on the CPU: the host split, the value classes, every
condition a case asserts on its reference (inside nt_case / tn_case), and the mutation table: the share of outputs
each dropped minor term of the six-term product changes, per oracle.  The GPU tests (tests/test_gpu_split_planes.py)
require the kernels to return these references bit for bit; this file shows, without a GPU, that a kernel which loses
any one of the five minor terms cannot.

To see the teeth: remove a term from split_oracles.TERMS (the emulation then loses it everywhere) and
test_nt_cases_meet_their_conditions / test_tn_cases_meet_their_conditions fail at every oracle that isolates it, at the
"six-term emulation != reference" condition; test_emulation_with_a_dropped_term_is_caught does the same per term."""
import pytest
import torch

import split_oracles as so

NT_SHAPES = [  # (kind, M, N, K, keywords) — the epilogues and the two-source A of the GPU cases, at host sizes
    ("fwd", 512, 256, 256, dict(accum=True)), ("fwd", 512, 256, 256, {}), ("plain", 512, 256, 256, {}),
    ("comb", 512, 256, 256, dict(prev=True)), ("lin", 300, 128, 128, {}), ("fwd", 300, 32, 128, dict(accum=True)),
    ("fwd", 256, 7, 64, {}), ("fwd", 200, 128, 100, {}), ("fwd", 512, 256, 512, dict(k1=256)),
    ("fwd", 512, 256, 512, dict(k1=256, off=256)), ("fwd", 384, 256, 384, dict(accum=True)),
]
TN_SHAPES = [(96 * 256 + 5, 256, 256), (16 * 256 + 1, 128, 512), (17, 256, 128), (1, 128, 128), (4101, 100, 77),
             (4101, 17, 128), (4101, 32, 128), (96 * 256 + 5, 128, 128)]


def test_host_split_of_the_classes():
    g = torch.Generator().manual_seed(3)
    for cls in ("T1", "T2", "T3"):
        v = so.values(cls, (4096,), g)
        so.occupancy(v, cls)
    v = so.values("T3", (4096,), g)
    p1, p2, p3 = so.host_split(v)
    s = torch.sign(v)
    assert bool(((p1 * s >= 1) & (p1 * s <= 3)).all()) and torch.equal(p1, torch.round(p1))
    assert torch.equal(p2 / so.Q10, torch.round(p2 / so.Q10)) and bool(((p2 * s / so.Q10 >= 2)).all())
    assert torch.equal(p3 / so.Q19, torch.round(p3 / so.Q19)) and bool(((p3 * s / so.Q19 >= 1)).all())
    # a dense random value: the three planes carry the whole significand but for the last bits
    x = torch.randn(4096, generator=g)
    q1, q2, q3 = so.host_split(x)
    assert bool(((q1.double() + q2.double() + q3.double() - x.double()).abs() <= 2.0 ** -24 * x.abs().double()).all())


def test_selectors_reach_every_column():
    g = torch.Generator().manual_seed(4)
    for width in (256, 128, 512, 77, 7):
        s = so.selector(width, width, "T1", g)
        assert sorted(s.c.tolist()) == list(range(width))
    s = so.row_selector(96 * 256 + 5, 256, 16, 1, "T1", g)
    assert s.r.numel() == 6 * 256 + 1 and bool((s.r // 16 == torch.arange(s.r.numel())).all())
    assert sorted(set((s.r % 16).tolist())) == list(range(16))                  # the live row's place rotates
    assert int(torch.bincount(s.c, minlength=256).max()) == 7


@pytest.mark.parametrize("oracle", so.NT_ORACLES)
def test_nt_cases_meet_their_conditions(oracle):
    for i, (kind, M, N, K, kw) in enumerate(NT_SHAPES):
        so.nt_case(oracle, kind, M, N, K, 100 + i, **kw)


@pytest.mark.parametrize("fused", (False, True))
@pytest.mark.parametrize("oracle", so.TN_ORACLES)
def test_tn_cases_meet_their_conditions(oracle, fused):
    for i, (M, N, K) in enumerate(TN_SHAPES):
        so.tn_case(oracle, M, N, K, 200 + i, fused)


def test_mutation_table(capsys):
    """Each minor term changes >= 99 % of the outputs of at least one oracle of each operation; the table is printed
    (pytest -s)."""
    rows = {("NT", o): so.nt_case(o, "fwd", 512, 256, 256, 7, accum=True)["table"] for o in so.NT_ORACLES}
    rows.update({("TN", o): so.tn_case(o, 96 * 256 + 5, 256, 256, 8, True)["table"] for o in so.TN_ORACLES})
    with capsys.disabled():
        print("\nshare of outputs changed by dropping one term")
        print("op oracle " + " ".join(f"{t:>7}" for t in so.MINOR))
        for (op, o), t in rows.items():
            print(f"{op} {o:<6} " + " ".join(f"{t[m]:7.4f}" for m in so.MINOR))
    for op in ("NT", "TN"):
        for term in so.MINOR:
            assert max(t[term] for (p, _), t in rows.items() if p == op) >= 0.99, (op, term)
    for (op, o), t in rows.items():                 # an oracle changes nothing under a term it does not hold
        for term in so.MINOR:
            if term not in so.ISOLATES[o]:
                assert t[term] == 0.0, (op, o, term)


@pytest.mark.parametrize("term", so.MINOR)
def test_emulation_with_a_dropped_term_is_caught(term):
    """The teeth: a six-term product that loses `term` is reported by every oracle that isolates it, NT and TN."""
    hit = 0
    for o in so.NT_ORACLES:
        c = so.nt_case(o, "plain", 512, 256, 256, 11)
        g = torch.Generator().manual_seed(11)
        a, w = c["in"]["a1"], c["in"]["w"]
        bad = so.six_terms(so.mm_nt, a, w, drop=(term,))
        if term in so.ISOLATES[o]:
            assert not torch.equal(bad, c["ref"]["c"]), (o, term)
            hit += 1
        else:
            assert torch.equal(bad, c["ref"]["c"]), (o, term)
    for o in so.TN_ORACLES:
        c = so.tn_case(o, 4101, 128, 128, 12, False)
        bad = so.six_terms(so.mm_tn, c["in"]["gy"], c["in"]["b"], drop=(term,))
        assert torch.equal(bad, c["ref"]["g_w"]) == (term not in so.ISOLATES[o]), (o, term)
    assert hit >= 1


def test_random_dense_operands_do_not_meet_the_conditions():
    """The conditions are not vacuous: randn operands fail the exactness condition."""
    g = torch.Generator().manual_seed(5)
    a, w = torch.randn(64, 256, generator=g), torch.randn(64, 256, generator=g)
    ref = so.mm_nt(a, w)
    with pytest.raises(AssertionError):
        so.exact_in_fp32(ref, so.mm_nt(a.abs(), w.abs()), so.Q19)
    with pytest.raises(AssertionError):
        so.occupancy(a, "T3")
