"""The wide DMA-staged kernels (conv_dma_kernel forward / dgrad, wgrad_dma_kernel) across ITEM boundaries inside a persistent block.

The DMA-vs-register-staged shapes of tests/test_gpu_conv.py give every persistent block at most one item, so nothing there crosses from
one (tile, M-block) item to the next inside a block: the item ring the loader waves publish and the consumers read after the barrier,
the pending epilogue of waves 4..7 that runs under the next item's first chunk, the bias / mask slots that rotate per item, the resident
weight chunk a K = 64 dgrad reuses across items, and the double-buffer parity of the weight-gradient kernel's tile loop with both copies
of that loop (the waves that also sum the bias gradient, and the others).  The shapes below are sized for that on a 256-CU part, and
each case first asks the library's own dispatch (mmif_conv2d_route) that its blocks really own several items, so a smaller part fails
loudly and never passes vacuously.

Harness of test_dma_staged_kernels_equal_register_staged: the same bf16 operands through both kernel generations
(mmif_debug_set_conv_dma 0 / 1); forward and dgrad run the same MFMA order and are bit identical, the weight gradient sums its tiles in
another order (2e-5); partial ReLU-mask and accumulate bit sets."""
import pytest
import torch

from gpu_util import close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (id, cin, cout, n, h, w, ops whose blocks must own more than three items / tiles, ops whose blocks must own more than one)
CASES = [
    # 832 items on 256 blocks: the item ring wraps, pending epilogues across items, both M-blocks
    ("128-128-13x128x128", 128, 128, 13, 128, 128, ("fwd", "dgrad"), ()),
    # ragged last tile row and column; consumer waves whose rows lie below the image
    ("128-128-13x100x120", 128, 128, 13, 100, 120, ("fwd", "dgrad"), ()),
    # the dgrad has K = 64, M = 128: two chunks per item, the resident weight chunks reused across items
    ("128-64-13x128x128", 128, 64, 13, 128, 128, ("dgrad",), ("fwd",)),
    # forward: ragged last chunk (11 channel blocks = 4 + 4 + 3) over several items per block; dgrad: ragged second M-block (88 of 128 rows)
    ("88-64-26x64x128", 88, 64, 26, 64, 128, ("dgrad",), ("fwd",)),
    # weight gradient: 64 tile groups per channel pair, four tiles per block -- double-buffer parity, both bias-role copies of the loop
    ("128-128-4x120x128", 128, 128, 4, 120, 128, ("wgrad",), ()),
    # weight gradient with a ragged last input-channel group (152 = 64 + 64 + 24) whose padded planes are not staged
    ("152-64-4x64x128", 152, 64, 4, 64, 128, (), ("wgrad",)),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_wide_kernels_across_item_boundaries(case):
    from mmif import tensor as T
    from mmif._lib import IMPL_MFMA, lib
    _, cin, cout, n, h, w, over3, over1 = case
    torch.manual_seed(cin * 7 + cout)
    x = T.BT.alloc(n, cin, h, w, torch.bfloat16, DEV); x.buf.normal_()
    gy = T.BT.alloc(n, cout, h, w, torch.bfloat16, DEV, halo=1, zero=True); gy.buf[:, :, 1:-1, 1:-1].normal_()
    gy = gy.as_folded()
    wt = torch.randn(cout, cin, 3, 3, device=DEV) * 0.05
    b = torch.randn(cout, device=DEV)
    pk = T.PackedWeights(cout, cin, 3, DEV); pk.pack(wt)
    ws = torch.empty(T.wgrad_workspace_bytes(cin, cout, 3) // 4 + 1, dtype=torch.float32, device=DEV)
    mask = 0x5a5a5a5a5a5a & ((1 << x.cb) - 1)
    acc_bits = 0x333333333333 & ((1 << x.cb) - 1)
    res = {}
    try:
        lib.mmif_debug_set_ragged(1)
        for mode in (0, 1):
            lib.mmif_debug_set_conv_dma(mode)
            y = T.BT.alloc(n, cout, h, w, torch.bfloat16, DEV)
            gx = T.BT.alloc(n, cin, h, w, torch.bfloat16, DEV, halo=1, zero=True)
            gx.buf.fill_(0.25)
            if mode == 1:   # what the DMA-staged launches below are, asked of the library for this device
                routes = {"fwd": T.conv_route("fwd", x, y, cin, cout, 3, impl=IMPL_MFMA),
                          "dgrad": T.conv_route("dgrad", gy, gx, cin, cout, 3, mask, acc_bits, impl=IMPL_MFMA),
                          "wgrad": T.conv_route("wgrad", x, gy, cin, cout, 3, impl=IMPL_MFMA)}
                for op, r in routes.items():
                    assert r is not None and r.name.startswith("wgrad_dma" if op == "wgrad" else "conv_dma"), (op, r)
                    print(f"{op}: {r.name} G {r.G} items {r.tiles}")
                for op in over3:
                    assert routes[op].tiles > 3 * routes[op].G, f"{op}: {routes[op]} -- no block owns more than three items on this device"
                for op in over1:
                    assert routes[op].tiles > routes[op].G, f"{op}: {routes[op]} -- no block owns a second item on this device"
            dw, db = torch.zeros_like(wt), torch.zeros_like(b)
            T.conv_fwd(x, wt, b, y, cin, cout, 3, True, pk, IMPL_MFMA)
            T.conv_dgrad(gy, wt, x, gx, cin, cout, 3, mask, acc_bits, pk, IMPL_MFMA)
            T.conv_wgrad(x, gy, dw, db, cin, cout, 3, ws, False, IMPL_MFMA)
            torch.cuda.synchronize()
            res[mode] = (y.buf.clone(), gx.buf.clone(), dw, db)
    finally:
        lib.mmif_debug_set_conv_dma(1)
        lib.mmif_debug_set_ragged(1)
    assert torch.equal(res[0][0], res[1][0]), "fwd differs"
    assert torch.equal(res[0][1], res[1][1]), "dgrad differs"
    close(res[1][2].cpu().numpy(), res[0][2].cpu().numpy(), 2e-5, "dw")
    close(res[1][3].cpu().numpy(), res[0][3].cpu().numpy(), 2e-5, "db")
