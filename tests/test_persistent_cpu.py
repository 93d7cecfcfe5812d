"""omniserve_amd.persistent.PersistentActivationBuffer hands out what the reference's layers expect to find in
`input_metadata.activation_buffer`: pinned against the reference's own class (omniserve/utils/input_metadata.py:18-112) through
tests/golden/activation_buffer.json (names, shapes, dtypes, strides, aliasing, sizes of its views), which is re-derived from
that class and must match where the reference tree is present; self-consistent everywhere.

    python -m tests.test_persistent_cpu      # rewrites tests/golden/activation_buffer.json (needs the reference tree)"""
import json
import os
import types

import pytest
import torch

from omniserve_amd.persistent import PersistentActivationBuffer
from tests import refstack

HID, INTER, QS, KVS = 256, 512, 256, 128


def _tensors(obj):
    return {k: v for k, v in vars(obj).items() if isinstance(v, torch.Tensor)}


def test_views_are_slices_of_one_allocation_and_alias_like_upstream():
    pab = PersistentActivationBuffer(HID, INTER, QS, KVS, max_tokens=300, chunk_prefill_size=128, device="cpu")
    seen = None
    for T in (1, 5, 128, 300):
        v = pab.view_for(T)
        assert v.qkv_proj_act_buffer.shape == (T, QS + 2 * KVS) and v.out_down_proj_act_buffer.shape == (T, HID)
        assert v.qkv_proj_act_buffer.data_ptr() == v.out_down_proj_act_buffer.data_ptr() == v.act_buffer.data_ptr()
        assert v.gate_up_proj_act_buffer.shape == (min(128, T), 2 * INTER)
        assert v.quantized_mlp_act_buffer.shape == (min(128, T), INTER) and v.quantized_mlp_act_buffer.dtype == torch.int8
        assert v.quantized_hidden_states_buffer.shape == (T, HID) and v.quantized_scale_buffer.shape == (T,)
        ptrs = tuple(t.data_ptr() for t in (v.act_buffer, v.gate_up_proj_act_buffer, v.quantized_act_buffer,
                                            v.quantized_mlp_act_buffer, v.quantized_scale_buffer, v.quantized_sum_buffer))
        assert seen is None or ptrs == seen, "a step view must not allocate"
        seen = ptrs
        assert all(t.is_contiguous() for t in _tensors(v).values())
    with pytest.raises(ValueError):
        pab.view_for(301)
    with pytest.raises(ValueError):
        pab.view_for(0)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "activation_buffer.json")
TOKENS = [1, 7, 128, 300]
# aliasing relations inside each object (offset from the fp16 / int8 base allocations)
ALIASES = (("act_buffer", ["qkv_proj_act_buffer", "out_down_proj_act_buffer"]),
           ("quantized_act_buffer", ["quantized_hidden_states_buffer"]))
SIZES = ("batched_seq_len", "hidden_size", "intermediate_size", "q_size", "kv_size", "chunk_prefill_size")


def _describe(buf):
    ts = _tensors(buf)
    return {"tensors": {n: [list(t.shape), str(t.dtype), list(t.stride())] for n, t in sorted(ts.items())},
            "alias_offsets": {n: ts[n].data_ptr() - ts[base].data_ptr() for base, names in ALIASES for n in names},
            "sizes": {n: getattr(buf, n) for n in SIZES}}


def _reference_view(T):
    with refstack.reference_over_mirror():
        from omniserve.utils.input_metadata import ActivationBuffer

        class LlamaForCausalLM:       # the class name is what upstream dispatches on (input_metadata.py:31-35)
            pass

        model = LlamaForCausalLM()
        model.model = types.SimpleNamespace(embed_tokens=types.SimpleNamespace(weight=torch.zeros((4, HID), dtype=torch.float16)))
        model.model_config = types.SimpleNamespace(chunk_prefill_size=128)
        model.q_size, model.kv_size = QS, KVS
        model.config = types.SimpleNamespace(intermediate_size=INTER, hidden_size=HID)
        ref = ActivationBuffer(model, T)
        ref.allocate_activation_buffer()
    return _describe(ref)


@pytest.mark.parametrize("T", TOKENS)
def test_view_matches_the_reference_activation_buffer(T):
    with open(GOLDEN) as f:
        want = json.load(f)[str(T)]
    if refstack.reference_available():
        assert _reference_view(T) == want, "tests/golden/activation_buffer.json is stale: python -m tests.test_persistent_cpu"
    assert all(off == 0 for off in want["alias_offsets"].values()), want["alias_offsets"]
    ours = _describe(PersistentActivationBuffer(HID, INTER, QS, KVS, max_tokens=300, chunk_prefill_size=128,
                                                device="cpu").view_for(T))
    assert set(ours["tensors"]) == set(want["tensors"]), (sorted(want["tensors"]), sorted(ours["tensors"]))
    for name, t in want["tensors"].items():
        assert ours["tensors"][name] == t, name
    assert ours["alias_offsets"] == want["alias_offsets"]
    for name in SIZES:
        assert ours["sizes"][name] == want["sizes"][name], name


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        json.dump({str(T): _reference_view(T) for T in TOKENS}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
