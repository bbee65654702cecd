"""The launch plan is pinned: every engine route (tests/launch_plan_cases.py: models x dtype x kernel family x A/B switch) calls the C entry
points golden F22 recorded, in that order, with those arguments.  The routes are bit-identical by design, so a step that silently takes a
fall-back fails no numeric test -- it fails here.  + the two pieces of hidden state the engines used to keep: the dup route's
flag on a cached lease, and the graph pins of chain_out's buffer pool."""
import gc
import json
import os
import weakref

import pytest
import torch

import launch_plan_cases as LP

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f22_launch_plans.json")


@pytest.fixture(scope="module")
def plans():
    with open(GOLDEN) as f:
        return json.load(f)["plans"]


def test_every_case_has_a_plan(plans):
    assert sorted(plans) == sorted(c["id"] for c in LP.CASES)


@pytest.mark.parametrize("case", LP.CASES, ids=[c["id"] for c in LP.CASES])
def test_launch_plan(case, plans):
    want = plans[case["id"]]
    got = LP.run_case(case)
    assert sorted(want) == sorted(str(s) for s in got)
    for step, calls in got.items():
        w, g = want[str(step)], LP.summarise(calls)
        if g == w:
            continue
        for i, c in enumerate(calls):         # the first call that differs, in full
            if i >= len(w["names"]) or g["names"][i] != w["names"][i] or g["calls"][6 * i:6 * i + 6] != w["calls"][6 * i:6 * i + 6]:
                exp = w["names"][i] if i < len(w["names"]) else "(nothing: the recorded plan ends here)"
                pytest.fail(f"{case['id']} step {step}: call {i} differs -- recorded: {exp}; now: {LP.canonical(c)}\n"
                            f"recorded names: {w['names']}\nnames now:      {g['names']}")
        pytest.fail(f"{case['id']} step {step}: {len(calls)} calls now, the recorded plan goes on with {w['names'][len(calls):]}")


def _densefuse_grads(m, imgs):
    for p in m.parameters():
        p.grad = None
    m(*imgs).square().mean().backward()
    torch.cuda.synchronize()
    return [p.grad.detach().clone() for p in m.parameters()]


def test_a_failed_backward_after_the_dup_route_leaves_no_state(monkeypatch):
    """DenseFuse, bf16: decode.0's dgrad also wrote the encoder branches' masked top blocks (the dup route), then the encoder backward
    raises.  The next step, with $MMIF_DGRAD_DUP=0, must run mmif_fuse_elem_bwd for those blocks: its gradients equal a fresh model's."""
    import core.model as M
    from mmif import tensor as T
    g = torch.Generator(device="cpu").manual_seed(5)
    imgs = [torch.rand(LP.SHARE_SHAPE, generator=g).to("cuda:0") for _ in range(2)]

    def model():
        torch.manual_seed(5)
        return M.DenseFuse().to("cuda:0")
    with LP.settings("bf16", "auto", {}):
        m = model()
        real = T.dense_encoder_bwd

        def boom(*a, **k):
            monkeypatch.setattr(T, "dense_encoder_bwd", real)
            raise RuntimeError("injected: the encoder backward fails once")
        monkeypatch.setattr(T, "dense_encoder_bwd", boom)
        with LP.record([]) as calls, pytest.raises(RuntimeError, match="injected"):
            m(*imgs).square().mean().backward()
        assert "mmif_conv2d_reflect_dgrad_folded_dup" in [c[0] for c in calls], "the step that failed did not take the dup route"
        assert T.dense_encoder_bwd is real
        with LP.settings("bf16", "auto", {"MMIF_DGRAD_DUP": "0"}):
            with LP.record([]) as calls:
                got = _densefuse_grads(m, imgs)
            assert "mmif_fuse_elem_bwd" in [c[0] for c in calls]
            want = _densefuse_grads(model(), imgs)
    assert len(got) == len(want) > 0
    for k, (a, b) in enumerate(zip(got, want)):
        assert float(b.abs().max()) > 0 and torch.equal(a, b), f"parameter {k}"


def test_graph_pins_die_with_their_buffers_and_the_pool_stays_bounded():
    """a pin lives on the pooled buffer it protects: dropping the buffers leaves no pin behind (the old module-level set of id()s pinned
    whatever later object got a recycled id, and chain_out's pool of unpinned shapes then grew past its bound)"""
    from mmif import engine as E
    from mmif.tensor import BT

    class Holder:       # stands in for the encoder's first ConvSpec: chain_out keeps its pool in the holder's __dict__
        pass
    dev = torch.device("cuda", 0)
    feats = [BT.alloc(1, 64, 16 + k, 16 + k, torch.bfloat16, dev) for k in range(12)]
    first = Holder()
    pinned = [E.DenseEncoderMixin.chain_out(first, F) for F in feats[:4]]
    for gz in pinned:
        E.pin_for_graph(gz)
    assert all(E.graph_pinned(gz) for gz in pinned)
    refs = [weakref.ref(gz.buf) for gz in pinned]
    del pinned, gz, first
    gc.collect()
    assert all(r() is None for r in refs), "a pinned buffer outlived its pool"
    # fresh allocations (which may land on the recycled ids / addresses) are not pinned, and 12 shapes leave at most 8 of them pooled
    first = Holder()
    for F in feats:
        assert not E.graph_pinned(E.DenseEncoderMixin.chain_out(first, F))
    assert sum(not E.graph_pinned(gz) for gz in first._gz.values()) <= 8
    keep = E.DenseEncoderMixin.chain_out(first, feats[0])        # a pinned buffer survives the same cycle
    E.pin_for_graph(keep)
    for F in feats[1:] + feats[1:]:
        E.DenseEncoderMixin.chain_out(first, F)
    assert any(gz is keep for gz in first._gz.values())
    assert sum(not E.graph_pinned(gz) for gz in first._gz.values()) <= 8
