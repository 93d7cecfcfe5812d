"""fused_ext.logprobs on the MI355X against the f64 oracle of its contract (tests/logprob_cases.py)."""
import numpy as np
import pytest
import torch

import logprob_cases as lc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _device_logits(case):
    x = torch.from_numpy(case.logits)
    if case.layout == "dense":
        return x.to(DEV)
    if case.layout == "strided":      # padded, odd row stride
        stride = case.cols + 24 + (case.cols % 2 == 0)
        buf = torch.full((case.rows, stride), float("nan"), dtype=torch.float16, device=DEV)
        buf[:, : case.cols] = x.to(DEV)
        assert buf.stride(0) % 2 == 1
        return buf[:, : case.cols]
    flat = torch.empty((case.rows * case.cols + 1,), dtype=torch.float16, device=DEV)      # base pointer 2-byte aligned only
    view = flat[1:].view(case.rows, case.cols)
    view.copy_(x.to(DEV))
    assert view.data_ptr() % 4 == 2
    return view


def _logprobs(logits, target, n_top):
    from omniserve_amd.backend import fused_ext
    out = fused_ext.logprobs(logits, target=torch.from_numpy(target).to(DEV), n_top=n_top)
    torch.cuda.synchronize()
    return out


def _argmax(logits):
    from omniserve_amd.backend import fused_ext
    out = torch.empty((logits.shape[0],), dtype=torch.int64, device=DEV)
    fused_ext.argmax(out, logits)
    return out


def _reference(case):
    """Per case, from the shared oracles: lse [rows], target log-probability / rank [rows], top tokens / log-probabilities."""
    orc = lc.case_oracles(case)
    lse = np.array([o.lse for o in orc])
    tgt = [o.target(int(case.target[r])) for r, o in enumerate(orc)]
    tops = [o.top(case.n_top) for o in orc]
    return (lse, np.array([t[0] for t in tgt]), np.array([t[1] for t in tgt]), np.stack([t[0] for t in tops]),
            np.stack([t[1] for t in tops]))


def test_case_grid_against_the_oracle():
    """Every row of every case (logprob_cases.cases(): cols 1 .. 128256 around the chunk and vector-load granularities, 1 / 3 / 16
    rows, dense / odd padded stride / 2-byte-aligned base, eleven profiles, eight target classes, n_top 0 / 1 / 5 / 20 and n_top >
    cols).  Tokens and ranks: equal, no tolerance; top_tokens[:, 0] bit-equal to fused_ext.argmax.  lse, token_logprob and
    top_logprobs: |err| <= 2e-5 + 2^-22 |ref|, with -inf, NaN and the -1 entries matched exactly.  Beside it, reported only: the
    error of torch.log_softmax(logits.float()) on the same rows.  Measured on the MI355X: largest |err| 3.48e-3 (a -65504 token
    under a 65504 maximum, |ref| = 131 009) = 0.122 of its bound; torch's f32 log-softmax on the same rows: 3.48e-3 = 0.111."""
    failures, worst_frac, worst_err, torch_frac, torch_err = [], 0.0, 0.0, 0.0, 0.0
    for case in lc.cases():
        logits = _device_logits(case)
        got = _logprobs(logits, case.target, case.n_top)
        lse, tlp, rank, top_tok, top_lp = _reference(case)
        if not np.array_equal(got.rank.cpu().numpy(), rank):
            failures.append("%s: ranks %s, oracle %s" % (case.name, got.rank.tolist(), rank.tolist()))
        if case.n_top:
            if not np.array_equal(got.top_tokens.cpu().numpy(), top_tok):
                failures.append("%s: top tokens differ from the oracle's" % case.name)
            if not torch.equal(got.top_tokens[:, 0], _argmax(logits)):
                failures.append("%s: top_tokens[:, 0] is not fused_ext.argmax" % case.name)
        else:
            assert got.top_tokens is None and got.top_logprobs is None
        for name, mine, ref in (("lse", got.lse, lse), ("token_logprob", got.token_logprob, tlp),
                                ("top_logprobs", got.top_logprobs, top_lp)):
            if mine is None:
                continue
            exact, frac, err = lc.value_errors(mine.cpu().numpy(), ref)
            if not exact:
                failures.append("%s: %s does not match the oracle's -inf / NaN entries" % (case.name, name))
            worst_frac, worst_err = max(worst_frac, frac), max(worst_err, err)
            if frac > 1.0:
                failures.append("%s: %s misses the bound by a factor %.3g (|err| %.3g)" % (case.name, name, frac, err))
        # torch's own f32 log-softmax on the same rows: the comparison, not the bar
        ref_rows = np.stack([o.logprob for o in lc.case_oracles(case)])
        ok = np.isfinite(ref_rows)
        if ok.any():
            tl = torch.log_softmax(logits.float(), dim=-1).cpu().numpy().astype(np.float64)
            e = np.abs(tl[ok] - ref_rows[ok])
            e = e[np.isfinite(e)]
            if e.size:
                torch_err = max(torch_err, float(e.max()))
                torch_frac = max(torch_frac, float((np.abs(tl[ok] - ref_rows[ok])[np.isfinite(tl[ok])] / lc.bound(ref_rows[ok][np.isfinite(tl[ok])])).max()))
    report = ("largest |err| %.3g = %.3g of its bound (torch.log_softmax in f32 on the same rows: %.3g = %.3g of the bound)" %
              (worst_err, worst_frac, torch_err, torch_frac))
    print(report)
    assert not failures, "%d failures, %s; first: %s" % (len(failures), report, "; ".join(failures[:6]))


def _bits(t):
    return t.view(torch.int32)


def test_same_bits_from_run_to_run_on_a_row_slice_and_whatever_n_top_is():
    rng = np.random.default_rng(9)
    for cols, pad in ((257, 0), (4104, 0), (4104, 16), (32000, 0)):      # (pad 16: a padded stride that keeps the 16-byte loads)
        rows = 5
        buf = torch.zeros((rows, cols + pad), dtype=torch.float16, device=DEV)
        buf[:, :cols] = torch.from_numpy((rng.standard_normal((rows, cols)) * 4).astype(np.float16)).to(DEV)
        logits = buf[:, :cols]
        target = rng.integers(0, cols, size=rows)
        a, b = _logprobs(logits, target, 20), _logprobs(logits, target, 20)
        for x, y in zip(a, b):
            assert torch.equal(_bits(x) if x.dtype == torch.float32 else x, _bits(y) if y.dtype == torch.float32 else y)
        z = _logprobs(logits, target, 0)
        assert torch.equal(_bits(a.lse), _bits(z.lse)) and torch.equal(_bits(a.token_logprob), _bits(z.token_logprob))
        assert torch.equal(a.rank, z.rank)
        five = _logprobs(logits, target, 5)
        assert torch.equal(five.top_tokens, a.top_tokens[:, :5]) and torch.equal(_bits(five.top_logprobs), _bits(a.top_logprobs[:, :5]))
        s = _logprobs(logits[1:], target[1:], 20)
        for x, y in zip(a, s):
            x = x[1:]
            assert torch.equal(_bits(x) if x.dtype == torch.float32 else x, _bits(y) if y.dtype == torch.float32 else y)
        # the same values in another layout (2-byte-aligned base: scalar loads): integer sums do not care
        flat = torch.empty((rows * cols + 1,), dtype=torch.float16, device=DEV)
        view = flat[1:].view(rows, cols)
        view.copy_(logits)
        m = _logprobs(view, target, 20)
        assert torch.equal(_bits(a.lse), _bits(m.lse)) and torch.equal(a.top_tokens, m.top_tokens)


def test_outputs_stay_inside_their_shapes_and_null_outputs_leave_the_others_alone():
    from omniserve_amd import _lib
    from omniserve_amd.backend import fused_ext
    rng = np.random.default_rng(10)
    rows, cols, n_top, guard = 3, 1000, 5, 2
    logits = torch.from_numpy((rng.standard_normal((rows + 2 * guard, cols)) * 3).astype(np.float16)).to(DEV)
    target = torch.from_numpy(rng.integers(0, cols, size=rows + 2 * guard)).to(DEV)
    poison_f, poison_i = -12345.0, -777
    lse = torch.full((rows + 2 * guard,), poison_f, dtype=torch.float32, device=DEV)
    tlp = torch.full_like(lse, poison_f)
    rank = torch.full((rows + 2 * guard,), poison_i, dtype=torch.int32, device=DEV)
    tt = torch.full((rows + 2 * guard, n_top), poison_i, dtype=torch.int64, device=DEV)
    tl = torch.full((rows + 2 * guard, n_top), poison_f, dtype=torch.float32, device=DEV)
    mid = slice(guard, guard + rows)
    fused_ext.logprobs(logits[mid], target=target[mid].contiguous(), n_top=n_top, lse=lse[mid], token_logprob=tlp[mid],
                       rank=rank[mid], top_tokens=tt[mid], top_logprobs=tl[mid])
    torch.cuda.synchronize()
    ref = fused_ext.logprobs(logits[mid], target=target[mid].contiguous(), n_top=n_top)
    for buf, r in ((lse, ref.lse), (tlp, ref.token_logprob), (rank, ref.rank), (tt, ref.top_tokens), (tl, ref.top_logprobs)):
        poison = poison_f if buf.dtype == torch.float32 else poison_i
        assert bool((buf[:guard] == poison).all()) and bool((buf[guard + rows:] == poison).all())      # guard rows
        assert torch.equal(buf[mid], r)
    # a narrower top list inside wider rows (a caller's [rows, 8] buffer is not this entry's business: columns are the row)
    # -- and each nullable output left null: the others as before, nothing else touched
    h = _lib.lib()
    ws = _lib.workspace(h.omni_logprob_workspace_bytes(rows, cols, n_top), torch.device(DEV), "logprob")
    x, t = logits[mid], target[mid].contiguous()
    for skip in ("lse", "tlp", "rank", "top"):
        o = dict(lse=torch.full((rows,), poison_f, dtype=torch.float32, device=DEV),
                 tlp=torch.full((rows,), poison_f, dtype=torch.float32, device=DEV),
                 rank=torch.full((rows,), poison_i, dtype=torch.int32, device=DEV),
                 tt=torch.full((rows, n_top), poison_i, dtype=torch.int64, device=DEV),
                 tl=torch.full((rows, n_top), poison_f, dtype=torch.float32, device=DEV))
        ptr = lambda name, off: None if off else o[name].data_ptr()      # noqa: E731
        rc = h.omni_logprob_f16(ptr("lse", skip == "lse"), ptr("tlp", skip == "tlp"), ptr("rank", skip == "rank"),
                                ptr("tt", skip == "top"), ptr("tl", skip == "top"), x.data_ptr(), x.stride(0), rows, cols,
                                t.data_ptr(), 0 if skip == "top" else n_top, ws.data_ptr(), ws.numel(), _lib.current_stream())
        assert rc == 0
        torch.cuda.synchronize()
        for name, r, off in (("lse", ref.lse, skip == "lse"), ("tlp", ref.token_logprob, skip == "tlp"),
                             ("rank", ref.rank, skip == "rank"), ("tt", ref.top_tokens, skip == "top"),
                             ("tl", ref.top_logprobs, skip == "top")):
            if off:
                assert bool((o[name] == (poison_f if o[name].dtype == torch.float32 else poison_i)).all()), (skip, name)
            else:
                assert torch.equal(o[name], r), (skip, name)
