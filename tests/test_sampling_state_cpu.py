"""runtime.SamplingState, the sampling parameters and draws that DecodeRunner and LServeDecodeRunner share, on the CPU device."""
import pytest
import torch

from omniserve_amd.lserve_runtime import LServeDecodeRunner
from omniserve_amd.runtime import DecodeRunner, SamplingState

B = 4


def _state(sampling=True, seed=7):
    s = SamplingState()
    s._init_sampling(sampling, B, torch.device("cpu"), seed)
    return s


def test_both_runners_use_the_one_implementation():
    for name in ("_init_sampling", "set_sampling", "_uniforms", "_refill_u", "_pick"):
        for cls in (DecodeRunner, LServeDecodeRunner):
            assert name not in vars(cls), "%s defines its own %s" % (cls.__name__, name)
            assert getattr(cls, name) is getattr(SamplingState, name)


def test_the_parameters_start_greedy():
    s = _state()
    assert s.sampling is True
    assert s.s_temperature.tolist() == [0.0] * B and s.s_temperature.dtype == torch.float32
    assert s.s_top_k.tolist() == [0] * B and s.s_top_k.dtype == torch.int32
    assert s.s_top_p.tolist() == [1.0] * B and s.s_top_p.dtype == torch.float32
    assert s.s_u.shape == (B,) and s.s_u.dtype == torch.float32


def test_a_scalar_and_a_per_row_value_reach_every_row_and_none_leaves_a_parameter_alone():
    s = _state()
    tensors = (s.s_temperature, s.s_top_k, s.s_top_p)
    s.set_sampling(temperature=0.5, top_k=[1, 2, 3, 4], top_p=torch.tensor([0.25, 0.5, 0.75, 1.0]))
    assert s.s_temperature.tolist() == [0.5] * B
    assert s.s_top_k.tolist() == [1, 2, 3, 4]
    assert s.s_top_p.tolist() == [0.25, 0.5, 0.75, 1.0]
    s.set_sampling(top_k=7)
    assert s.s_temperature.tolist() == [0.5] * B and s.s_top_k.tolist() == [7] * B and s.s_top_p.tolist() == [0.25, 0.5, 0.75, 1.0]
    s.set_sampling()
    assert s.s_temperature.tolist() == [0.5] * B and s.s_top_k.tolist() == [7] * B and s.s_top_p.tolist() == [0.25, 0.5, 0.75, 1.0]
    assert all(a is b for a, b in zip(tensors, (s.s_temperature, s.s_top_k, s.s_top_p)))      # written in place
    with pytest.raises(RuntimeError):
        s.set_sampling(top_k=[1, 2, 3])                                                         # neither one value nor B


def test_set_sampling_on_a_greedy_runner_raises():
    s = _state(sampling=False)
    assert s.sampling is False and not hasattr(s, "s_u")
    with pytest.raises(RuntimeError, match="sampling=True"):
        s.set_sampling(temperature=1.0)
    s._refill_u()                                                                               # nothing to refill: no error


def test_the_same_seed_gives_the_same_uniforms():
    a, b = _state(seed=7), _state(seed=7)
    ua = a._uniforms(2, B, 3)
    assert ua.shape == (2, B, 3) and ua.dtype == torch.float32 and bool(((ua >= 0) & (ua < 1)).all())
    assert torch.equal(ua, b._uniforms(2, B, 3))
    a._refill_u()
    b._refill_u()
    assert torch.equal(a.s_u, b.s_u) and not torch.equal(a.s_u, torch.zeros(B))
    want = torch.rand((B,), generator=torch.Generator().manual_seed(3))
    a.set_sampling(seed=3)
    a._refill_u()
    assert torch.equal(a.s_u, want)                                                             # one (B,) draw per refill
    assert not torch.equal(_state(seed=8)._uniforms(B), _state(seed=7)._uniforms(B))


def test_a_greedy_pick_is_the_arg_max():
    s = _state(sampling=False)
    s.tokens = torch.zeros((B,), dtype=torch.int64)
    logits = torch.randn((B, 32), generator=torch.Generator().manual_seed(0)).half()
    s._pick(logits, fused_argmax=False)
    assert torch.equal(s.tokens, torch.argmax(logits, dim=-1))
