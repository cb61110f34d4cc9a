"""The float16 device rollout without a GPU: the precision keyword's refusal and the alignment a plan built on fp16 slab
strides gives every task (the two C-ABI symbols in the header and the binding: tests/test_abi.py)."""
import numpy as np
import pytest

from coevonet_amd import lib as L
from coevonet_amd.rollout import DeviceRollout, RolloutPlan


def test_unknown_precision_raises_before_the_library_is_loaded(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(L, "load", no_load)
    for bad in ("bfloat16", "half", "", None):
        with pytest.raises(ValueError, match="Unsupported precision"):
            DeviceRollout(None, None, precision=bad)


def test_plan_on_fp16_strides_keeps_every_net_offset_16_byte_aligned():
    s10, s8 = L.fc16_slab_stride(10), L.fc16_slab_stride(8)
    assert s10 % 64 == 0 and s8 % 64 == 0
    npop, nh = 7, 3
    n10 = 2 * (npop + nh)
    off = [i * s10 for i in range(n10)] + [n10 * s10 + k * s8 for k in range(npop + nh)]
    D = [10] * n10 + [8] * (npop + nh)
    games = [(n10 + npop + k, i, npop + nh + npop + k) for i in range(npop) for k in range(nh)]
    games += [(n10 + i, npop + k, npop + nh + npop + k) for i in range(npop) for k in range(nh)]
    plan = RolloutPlan(np.array(games), off, D, device=None, heavy_rows=16, n_cohorts=2)
    offs = np.concatenate([plan.heavy_np["net_off"], plan.light_np["net_off"]])
    assert len(offs) and (offs % 4 == 0).all()
