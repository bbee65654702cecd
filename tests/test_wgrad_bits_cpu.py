"""The table of golden F23 (tests/wgrad_bits_cases.py) reaches what it claims, without a GPU: every reduce flavour in both regimes of the
fixed-order sum (where the flavour's slice rule lets G reach them) with accumulate off and on, every flavour whose wrapper takes db = None
without db; and the fixture holds exactly the table's cases, none with an all-zero output."""
import json
import os

import wgrad_bits_cases as B

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f23_wgrad_bits.json")


def test_every_flavour_in_both_regimes_with_accumulate_off_and_on():
    reached = {}
    for c in B.CASES:
        for flavour, G, sl in c.reduces:
            assert sl in (4, 16) and G >= 1, c.id
            if flavour.startswith(("wgrad_dma", "wgrad_x3_reduce", "reduce_multi_kernel wgrad_dma")):
                assert sl == (16 if G > 64 else 4), f"{c.id}: the slice count of {flavour} follows G"
            reached.setdefault(flavour, set()).add((B.regime(G, sl), c.accumulate))
    assert len(reached) >= 20
    missing = [(f, r, a) for f in sorted(reached) for r in ("tail", "main+tail") for a in (0, 1)
               if (r, a) not in reached[f] and (f, r) not in B.UNREACHABLE and not f.startswith("reduce_multi_kernel")]
    # (the deferred sequence runs one launch of four jobs: an SL-4 and an SL-16 job, all main+tail; its maps' other regimes are the single launches')
    assert not missing, missing
    for f, r in B.UNREACHABLE:
        assert f in reached and all(rr != r for rr, _ in reached[f]), (f, r)
    multi = {f: v for f, v in reached.items() if f.startswith("reduce_multi_kernel")}
    assert {f.rsplit("/", 1)[1] for f in multi} == {"4", "16"} and all({a for _, a in v} == {0, 1} for v in multi.values())


def test_db_not_wanted_is_covered_per_entry_point():
    ops = {c.op for c in B.CASES}
    assert ops == {"wgrad", "bwd_pair", "bwd_wide", "image_in_wgrad", "image_out_wgrad", "image_out_bwd", "dense_encoder_wgrad", "dense_encoder_bwd", "deferred"}
    assert {c.op for c in B.CASES if not c.db} == ops - {"deferred"}


def test_G_follows_the_launchers_formulas():
    """spot values worked by hand from the launchers (16 x 16 tiles unless said); the ConvLayer calls' pin what the library answers"""
    assert B.G_dma(64, 64, 3, 80, 96) == 90 and B.G_dma(64, 136, 3, 80, 96) == 80 and B.G_dma(64, 64, 2, 33, 40) == 18
    assert B.G_mfma(20, 12, 3, 1, 33, 40) == 9 and B.G_mfma(88, 64, 1, 2, 33, 40) == 18
    assert B.G_taprow(48, 16, 2, 33, 40) == 18 and B.G_taprow(48, 16, 3, 80, 96) == 90 and B.G_pair(64, 3, 80, 96) == 90
    assert B.G_dma(64, 64, 9, 128, 128) == 256 and B.G_mfma(20, 12, 3, 9, 128, 128) == 384 and B.G_pair(32, 9, 128, 128) == 512     # the caps
    import conv_cases as CC
    assert CC.route("bwd_pair", "bf16", 32, 16, 2, 256, 257, num_cus=304).G == 512, "544 tiles on 304 compute units: the workspace holds 512 partials"
    assert B.G_x3(64, 64, 3, 2, 40, 96) == 60 and B.G_x3(72, 40, 1, 1, 80, 48) == 90          # 8 x 16 tiles; 1x1: three partials per block
    assert B.G_x3_thin(48, 3, 40, 96) == 90 and B.G_x3_dense(2, 33, 40) == 30
    assert B.G_image(3, 80, 96) == 90 and B.G_image(2, 33, 40) == 11                          # 256 pixels per block
    assert B.G_image_bwd(3, 80, 96) == 88 and B.G_image_bwd(2, 33, 40) == 16                  # 8 x 32 tiles, rounded down to a multiple of 8
    assert B.G_enc_bwd(3, 80, 96, 1) == 30 and B.G_enc_bwd(8, 144, 40, 2) == 72


def test_fixture_holds_exactly_the_table():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert g["num_cus"] == B.NUM_CUS and len(g["commit"]) >= 7
    assert sorted(g["cases"]) == sorted(c.id for c in B.CASES)
    for cid, rec in g["cases"].items():
        assert len(rec["inputs"]) == 64 and rec["outputs"], cid
        for name, o in rec["outputs"].items():
            assert len(o["sha256"]) == 64 and o["sum"] != 0.0, f"{cid} {name}: an all-zero output pins nothing"


def test_conv_wgrad_cases_take_the_route_their_flavour_names():
    """the library's dispatch (conv_cases.expected_kernel asks mmif_conv2d_route) for every conv_wgrad case of the table, and the slice
    count of its reduce"""
    import conv_cases as CC
    want = {"wgrad_dma_reduce": "wgrad_dma", "taprow_wgrad_reduce": "wgrad_taprow", "wgrad_x3_thin_reduce": "x3_wgrad_thin<6>"}
    routes = set()
    for c in B.CASES:
        if c.op != "wgrad":
            continue
        route = CC.expected_kernel("wgrad", c.dtype, c.cin, c.cout, c.n, c.h, c.w, k=c.k, impl="x3" if c.dtype == "f32" else "mfma")
        flavour = c.reduces[0][0].split("/")[0].split("<")[0]
        if flavour == "wgrad_mfma_reduce":
            ks, mfw, icf = c.reduces[0][0].split("<")[1].split(">")[0].split(",")
            assert route == (f"wgrad_mfma<3,{mfw}>" if ks == "3" else f"wgrad_mfma<1,{mfw},2,{icf}>"), (c.id, route)
        else:
            assert route == (f"x3_wgrad<{c.k}>" if flavour == "wgrad_x3_reduce" else want[flavour]), (c.id, route)
        r = CC.route("wgrad", c.dtype, c.cin, c.cout, c.n, c.h, c.w, k=c.k, impl="x3" if c.dtype == "f32" else "mfma", num_cus=B.NUM_CUS)
        assert (r.G, r.slices) == c.reduces[0][1:], (c.id, r)
        if flavour == "wgrad_x3_thin_reduce":
            assert c.cin <= 48 and c.cout <= 16 and c.k == 3, c.id
        routes.add(route)
    assert {"wgrad_dma", "wgrad_taprow", "wgrad_mfma<3,1>", "wgrad_mfma<3,4>", "wgrad_mfma<1,4,2,4>", "wgrad_mfma<1,4,2,2>", "x3_wgrad<3>", "x3_wgrad<1>",
            "x3_wgrad_thin<6>"} <= routes
