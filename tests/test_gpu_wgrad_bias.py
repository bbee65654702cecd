"""Which blocks of wgrad_dma_kernel sum the bias gradient (csrc/conv_mfma.hip, mmif_debug_set_wgrad_bias).

The reduce reads db from the blocks of input-channel group 0 only, so the blocks of the other groups neither compute nor store bias
sums (setter 1, the default); setter 0 has every block do it, as before.  The blocks that keep the work run the same MFMAs on the same
operands in the same order: dW, db and the ReLU sign bytes must be BIT-IDENTICAL between the two, and dW / db must match the fp64
definition on the bf16-rounded operands -- a fragment-to-channel mix-up common to both would pass the first check and fail the second.

Shapes: one or several input groups (192 -> 64: two groups without bias work), ragged last groups (88 -> 120, 152 -> 64), one tile,
ragged tiles in both directions, several tiles; batch 1 and 3; a shrunk persistent grid for several tiles per block; the plain weight
gradient and the one of mmif_conv2d_reflect_bwd_wide that also leaves the sign bytes.  The partial-sum workspace is poisoned with NaN
before every launch: a slot the kernel no longer writes but the reduce still read would show in dW / db."""
import pytest
import torch

from gpu_util import DEV, close, dtype_ctx

pytestmark = pytest.mark.gpu

CHANNELS = [(128, 64), (64, 128), (128, 128), (192, 64), (88, 120), (152, 64)]
IMAGES = [(16, 16), (17, 33), (48, 32)]
MODES = (0, 1)


def _operands(cin, cout, n, h, w):
    from mmif import tensor as T
    g = torch.Generator().manual_seed(cin * 1009 + cout * 31 + n * 7 + h * 3 + w)
    x = T.BT.from_nchw(torch.randn(n, cin, h, w, generator=g).to(DEV), torch.bfloat16)
    gy = T.BT.from_nchw(torch.randn(n, cout, h, w, generator=g).to(DEV), torch.bfloat16, halo=1).as_folded()
    wt = (torch.randn(cout, cin, 3, 3, generator=g) * 0.05).to(DEV)
    return x, gy, wt


def _all_modes(run):
    """run() under both settings of the bias switch, the workspace poisoned first; the library's default restored afterwards"""
    from mmif._lib import lib
    res = {}
    try:
        for mode in MODES:
            lib.mmif_debug_set_wgrad_bias(mode)
            res[mode] = run()
            torch.cuda.synchronize()
    finally:
        lib.mmif_debug_set_wgrad_bias(1)
    return res


def _check(cin, cout, n, h, w, min_tiles_per_block=1):
    from mmif import tensor as T
    from mmif._lib import IMPL_MFMA
    with dtype_ctx("bf16"):
        x, gy, wt = _operands(cin, cout, n, h, w)
        r = T.conv_route("wgrad", x, gy, cin, cout, 3, impl=IMPL_MFMA)
        assert r is not None and r.name.startswith("wgrad_dma"), r
        assert r.tiles >= min_tiles_per_block * r.G, f"{r}: the blocks own fewer than {min_tiles_per_block} tiles each"
        ws = torch.empty(T.wgrad_workspace_bytes(cin, cout, 3) // 4 + 1, dtype=torch.float32, device=DEV)

        # ---- the plain weight gradient
        def plain():
            ws.fill_(float("nan"))
            dw, db = torch.zeros(cout, cin, 3, 3, device=DEV), torch.zeros(cout, device=DEV)
            T.conv_wgrad(x, gy, dw, db, cin, cout, 3, ws, False, IMPL_MFMA)
            return dw, db
        res = _all_modes(plain)
        assert torch.equal(res[0][0], res[1][0]), "dW: setter 0 differs from the default"
        assert torch.equal(res[0][1], res[1][1]), "db: setter 0 differs from the default"

        # ---- the fp64 definition on the same bf16 operands (reflect-padded x, interior of gy)
        xs, gs = x.to_nchw().double(), gy.to_nchw().double()
        ref_dw = torch.nn.grad.conv2d_weight(torch.nn.functional.pad(xs, (1, 1, 1, 1), mode="reflect"), wt.shape, gs)
        ref_db = gs.sum(dim=(0, 2, 3))
        e_dw = close(res[1][0].cpu().numpy(), ref_dw.cpu().numpy(), 1e-4, "dw vs fp64")
        e_db = close(res[1][1].cpu().numpy(), ref_db.cpu().numpy(), 1e-4, "db vs fp64")
        print(f"{cin}->{cout} {n}x{h}x{w}: {r.name} G {r.G} tiles {r.tiles}; dw err {e_dw:.2e}, db err {e_db:.2e}")

        # ---- the weight gradient that also leaves the sign bytes (layers of whole 64-channel groups)
        if not T.bwd_wide_supported(cin, cout, 3):
            assert cin % 64 or cout % 64
            return
        pk = T.PackedWeights(cout, cin, 3, DEV)
        pk.pack(wt)

        def wide():
            ws.fill_(float("nan"))
            signs = torch.full((T.bwd_wide_signs_bytes(n, cin, h, w),), 0xA5, dtype=torch.uint8, device=DEV)
            gx = T.BT.alloc(n, cin, h, w, torch.bfloat16, DEV, halo=1, zero=True)
            dw, db = torch.zeros(cout, cin, 3, 3, device=DEV), torch.zeros(cout, device=DEV)
            T.conv_bwd_wide(gy, x, gx, dw, db, cin, cout, 3, pk, (1 << (cin // 8)) - 1, ws, signs)
            return dw, db, signs, gx.buf
        wres = _all_modes(wide)
        for i, what in enumerate(("dW", "db", "sign bytes", "gx")):
            a, b = wres[0][i], wres[1][i]
            if what == "gx":
                a, b = a.view(torch.int16), b.view(torch.int16)
            assert torch.equal(a, b), f"bwd_wide {what}: setter 0 differs from the default"
        # the sign-byte launch is the plain one plus the bytes
        assert torch.equal(wres[1][0], res[1][0]) and torch.equal(wres[1][1], res[1][1])
        # the bytes themselves: [n][cb][h + 2][pitch], byte of padded column X at X + 15, bit i = channel 8 cb + i > 0
        pitch = ((w + 15) // 16 + 2) * 16
        sg = wres[1][2].view(n, cin // 8, h + 2, pitch)[:, :, 1:h + 1, 16:16 + w]
        pos = x.buf.float() > 0
        want = (pos.to(torch.int32) << torch.arange(8, device=pos.device, dtype=torch.int32)).sum(-1).to(torch.uint8)
        assert torch.equal(sg, want)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("h,w", IMAGES, ids=[f"{h}x{w}" for h, w in IMAGES])
@pytest.mark.parametrize("cin,cout", CHANNELS, ids=[f"{a}-{b}" for a, b in CHANNELS])
def test_bias_only_in_input_group_0_agrees_and_matches_fp64(cin, cout, n, h, w):
    _check(cin, cout, n, h, w)


@pytest.mark.parametrize("blocks", [8, 32])
@pytest.mark.parametrize("cin,cout", [(128, 64), (192, 64), (152, 64)], ids=["128-64", "192-64", "152-64"])
def test_bias_only_in_input_group_0_with_several_tiles_per_block(cin, cout, blocks):
    """At the shapes above every block owns one tile (the grid shrinks to the tile count).  A smaller persistent grid
    (mmif_debug_set_wgrad_dma_blocks) gives each block 2 to 18 tiles of a 4 x 48 x 33 batch: both halves of the double buffer, both
    copies of the tile loop over several tiles, tile counts that differ between blocks; 8 blocks also leave the XCD-aware block order."""
    from mmif._lib import lib
    try:
        lib.mmif_debug_set_wgrad_dma_blocks(blocks)
        _check(cin, cout, 4, 48, 33, min_tiles_per_block=2)
    finally:
        lib.mmif_debug_set_wgrad_dma_blocks(256)
