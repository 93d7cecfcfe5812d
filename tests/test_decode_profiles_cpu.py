"""CPU-side checks of tests/decode_score_profiles.py: its f64 expected values against the decode oracle on ordinary inputs, the
fairness of every case (an f32 softmax of the oracle's kind fits in half the project's 1e-3 bar), and that the planted tokens
really dominate.  No GPU."""
import numpy as np
import pytest

from tests import decode_score_profiles as dp
from tests.util import attention_errors

FAIR = 5e-4        # half of tests.util.assert_attention_close's bar: the kernel keeps the other half


@pytest.mark.parametrize("spec", dp.RANDOM_SPECS, ids=[s[0] for s in dp.RANDOM_SPECS])
def test_expected_builder_is_the_decode_oracle_on_random_inputs(spec):
    """N(0, 1) q, k, v and history: the same keys, values, RoPE and normaliser 1 / (sum + 1e-6) as
    oracle.kv4.decode_attention(emulate_fp16=False); the two differ in f32 against f64 score / softmax arithmetic only.  The
    argument of tests/test_paged_prefill_cpu.py::test_expected_builder_with_one_query_is_the_decode_oracle for the same pair: the
    f32 roundings of a few hundred products and sums are a few 1e-7 of the head's largest element BEFORE each side's final
    rounding to fp16, so after it every element agrees to 1e-5 of the head's largest element or is the neighbouring fp16 value,
    and the neighbours are rare (under 5 % of the elements)."""
    c = dp.random_case(spec)
    want16, raw = c.oracle_f32()
    got, want = c.want.astype(np.float64), want16.astype(np.float64)
    head_max = np.abs(want).max(axis=-1, keepdims=True)
    close = np.abs(got - want) <= 1e-5 * head_max
    neighbour = np.abs(got - want) <= np.spacing(np.abs(want16)).astype(np.float64) * 1.0000001
    print("elements beyond 1e-5: %d of %d" % ((~close).sum(), close.size))
    assert (close | neighbour).all(), "max |d| / head max = %.3g" % float((np.abs(got - want) / head_max).max())
    assert (~close).mean() < 0.05
    assert np.abs(raw.astype(np.float64) - c.want64).max() <= 1e-5 * head_max.max()


@pytest.mark.parametrize("name", list(dp.DENSE) + list(dp.MERGE))
def test_every_case_is_fair(name):
    """A CONDITION on the case, not a tolerance on the kernel: oracle.kv4.decode_attention(emulate_fp16=False) -- f32 scores, f32
    softmax, the arithmetic class of the kernel -- must land within 5e-4 (tests.util.attention_errors) of the f64 expected
    values.  A profile that does not is shrunk in tests/decode_score_profiles.py; the bar is not raised.

    The distance is taken on the values BEFORE each side's final rounding to fp16.  After it, two values 1e-6 apart that sit
    astride a rounding boundary come out one fp16 step apart, and one step at a head's largest element is up to 2^-10 = 9.8e-4 of
    it: that says nothing about the f32 arithmetic (ordinary N(0, 1) cases show the same flips) and would make the condition a
    coin toss.  The rounded outputs are still held to: rel L2 <= 5e-4 (a flip does not move it), and every element within 5e-4 of
    the head's largest element OR the neighbouring fp16 value."""
    c = dp.case(name)
    o16, raw = c.oracle_f32()
    l2, linf = attention_errors(raw, c.want64)
    l2r, linfr = attention_errors(o16.astype(np.float32), c.want.astype(np.float32))
    print("fairness %-16s %-64s unrounded: rel L2 %.2e  max |d| / head max %.2e   fp16: %.2e / %.2e" % (
        name, c.seqs, l2, linf, l2r, linfr))
    assert l2 <= FAIR and linf <= FAIR
    assert l2r <= FAIR
    got, want = o16.astype(np.float64), c.want.astype(np.float64)
    head_max = np.abs(want).max(axis=-1, keepdims=True)
    close = np.abs(got - want) <= FAIR * head_max
    neighbour = np.abs(got - want) <= np.spacing(np.abs(c.want)).astype(np.float64) * 1.0000001
    assert (close | neighbour).all()
    assert name in dp.FAIRNESS, "record the measured distance in decode_score_profiles.FAIRNESS"


@pytest.mark.parametrize("name", [n for n in list(dp.DENSE) + list(dp.MERGE)
                                  if any(s.kind == "needle" for s in (dp.DENSE.get(n) or dp.MERGE[n])[1])])
def test_needles_are_needles(name):
    c = dp.case(name)
    assert c.needles
    for b, nt in c.needles:
        for hk in range(c.Hk):
            w = c.weights[(b, hk * c.g)]
            assert w[nt] >= 0.99, "%s: sequence %d, kv head %d: the planted token %d holds %.4f of the weight" % (
                name, b, hk, nt, w[nt])
            assert int(np.argmax(w)) == nt


def test_flat_exact_weights_are_equal_and_profiles_have_their_shape():
    """flat_exact: identical K rows -> bit-identical scores -> exactly equal history weights.  climb: the gain-1 head's scores rise
    by at least 1 per 32-token tile over a range of ~60 (log-weights, as the reference reads them back from the 4-bit pages);
    offset: the common shift really is ~200."""
    name = next(n for n, s in dp.DENSE.items() if n.startswith("pipe2") and any(q.kind == "flat_exact" for q in s[1]))
    c = dp.case(name)
    b = next(i for i, s in enumerate(c.seqs) if s.kind == "flat_exact")
    w = c.weights[(b, 0)][:-1]
    assert (w == w[0]).all() and w[0] > 0
    name = next(n for n, s in dp.DENSE.items() if n.startswith("pipe2") and any(q.kind == "climb" for q in s[1]))
    c = dp.case(name)
    b = next(i for i, s in enumerate(c.seqs) if s.kind == "climb")
    lw = np.log(c.weights[(b, 0)][:-1])
    tiles = lw[: len(lw) // 32 * 32].reshape(-1, 32).max(axis=1)
    assert (np.diff(tiles) >= 1.0).all() and 55.0 <= lw.max() - lw.min() <= 65.0


def test_split_tokens_matches_the_geometries_the_tables_name():
    assert dp.split_tokens(701, 7) == 112 and dp.split_tokens(1401, 2) == 704 and dp.split_tokens(1201, 2) == 608
    assert 608 == 38 * 16                       # window2: 38 of the 40 page-window pointers
    assert dp.split_tokens(701, 7) % 32 != 0    # a ragged last tile in every split
    assert dp.split_tokens(1401, 2) > 640 >= dp.split_tokens(701, 7)      # PIPE above 640 tokens per split, the short form below
    for name, (n, seqs, Hq, Hk, tpb, ns) in list(dp.DENSE.items()) + list(dp.MERGE.items()):
        ctx = max(s.T for s in seqs) + 1
        assert len(seqs) <= 3 and ns <= (ctx + 63) // 64, name      # the wrapper's workspace covers the forced count
