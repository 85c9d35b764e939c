"""Pins tests/ultra_ref.py (the references and input generators of tests/test_gpu_ultra_kernels.py) on the CPU:
the restatements reproduce the oracles, and for every GPU parametrisation the reference alone meets the conditions
the tie-proven comparison needs: the possible ties stay within their cap and the codes spread."""
import numpy as np
import pytest
import torch

import ultra_ref as R
from oracle import quantization_np as Q
from oracle import ultranet_oracle as U


def _block_sd(k, cin, cout, ks, seed):
    g = torch.Generator().manual_seed(seed)
    cp, bp = U.layer_prefixes()[k]
    return {cp + ".weight": torch.randn(cout, cin, ks, ks, generator=g) * 0.3,
            bp + ".weight": torch.rand(cout, generator=g) + 0.5, bp + ".bias": torch.randn(cout, generator=g) * 0.2 + 0.4,
            bp + ".running_mean": torch.randn(cout, generator=g) * 0.1,
            bp + ".running_var": torch.rand(cout, generator=g) * 0.5 + 0.05}, cp, bp


def _fold(sd, bp, eps=1e-5):
    a = sd[bp + ".weight"].double() / torch.sqrt(sd[bp + ".running_var"].double() + eps)
    return a.float(), (sd[bp + ".bias"].double() - sd[bp + ".running_mean"].double() * a).float()


def _oracle_codes(sd, k, x):
    """ultranet_block in float64 (the fp32 oracle's own conv rounding is not part of the kernels' contract)."""
    y = U.ultranet_block({n: t.double() for n, t in sd.items()}, k, x.double())
    return torch.round(y * 15).to(torch.int64).permute(0, 2, 3, 1)


@pytest.mark.parametrize("k", [1, 4])
def test_codes_ref_reproduces_oracle_block(k):
    cin, cout, ks, pool = U.CONV_SPECS[k]
    sd, cp, bp = _block_sd(k, cin, cout, ks, 40 + k)
    sd[bp + ".weight"] = sd[bp + ".weight"] * 0.25           # conv values k/15 * k/7 over 9 cin taps: spread, not saturate
    alpha, shift = _fold(sd, bp)
    x = R.gen_codes((2, 12, 10, cin), 4, 7)
    w = U.weight_codes(sd[cp + ".weight"], 4).to(torch.int64).permute(0, 2, 3, 1).contiguous()
    codes, tie = R.codes_ref(R.conv_acc(x, w), R.den_of(4, 4), alpha, shift, 15, pool)
    want = _oracle_codes(sd, k, x.permute(0, 3, 1, 2).double() / 15)
    assert len(torch.unique(want)) >= 8 and R.tie_share(tie) <= R.CAP_INT_ACC
    assert torch.equal(codes[~tie], want[~tie])
    assert (codes - want).abs().max() <= 1


def test_conv0_ref_reproduces_oracle_block():
    sd, cp, bp = _block_sd(0, 3, 16, 3, 50)
    alpha, shift = _fold(sd, bp)
    img = torch.rand(2, 3, 17, 22, generator=torch.Generator().manual_seed(3))
    codes, tie = R.conv0_ref(img, U.weight_quantize(sd[cp + ".weight"]), alpha, shift, 15)
    want = _oracle_codes(sd, 0, img)
    assert codes.shape == (2, 8, 11, 16)
    assert len(torch.unique(want)) >= 8 and R.tie_share(tie) <= R.CAP_CONV0
    assert torch.equal(codes[~tie], want[~tie])
    assert (codes - want).abs().max() <= 1


def test_conv0_int_ref_equals_oracle_first_layer():
    g = torch.Generator().manual_seed(8)
    arrs, specs = {}, [(c[0], c[1], c[2]) for c in U.CONV_SPECS]
    n = 0
    for cin, cout, ks in specs:
        for a in (torch.randn(cout, cin, ks, ks, generator=g) * 0.3, torch.rand(cout, generator=g) + 0.5,
                  torch.randn(cout, generator=g) * 0.2 + 0.3, torch.randn(cout, generator=g) * 0.1,
                  torch.rand(cout, generator=g) * 0.5 + 0.05, torch.tensor(1e-5)):
            arrs[f"arr_{n}"] = a.numpy()
            n += 1
    arrs[f"arr_{n}"] = (torch.randn(36, 64, 1, 1, generator=g) * 0.3).numpy()
    arrs[f"arr_{n + 1}"] = torch.randn(36, generator=g).numpy()
    arrs["arr_1"] = arrs["arr_1"] * 0.02                      # layer 0 sees pixels 0..255: spread, not saturate
    img = torch.randint(0, 256, (3, 16, 16), generator=g, dtype=torch.uint8)
    want = Q.ultranet_int_forward(arrs, img.numpy())[0]
    w = Q.weight_quantize_int(arrs["arr_0"], 4)
    inc, bias = Q.bn_act_quantize_int(*(arrs[f"arr_{i}"] for i in range(1, 6)), w_bit=4, in_bit=8, out_bit=4, l_shift=8)
    got = R.conv0_int_ref(img[None], torch.from_numpy(w), torch.from_numpy(inc), torch.from_numpy(bias), 19, 4)
    assert np.array_equal(R.conv0_int_acc(img[None], torch.from_numpy(w))[0].permute(2, 0, 1).numpy(),
                          Q.conv_int(img.numpy().astype(np.int64), w, 1))
    assert len(np.unique(want)) >= 8
    assert np.array_equal(got[0].permute(2, 0, 1).numpy(), want)


def test_conv_acc_equals_conv_int_in_fp32_too():
    x = R.gen_codes((1, 9, 7, 64), 7, 1)
    w = torch.randint(-127, 128, (20, 3, 3, 64), generator=torch.Generator().manual_seed(2))
    w[0] = 127                                               # one channel near the largest accumulator
    want = Q.conv_int(x[0].permute(2, 0, 1).numpy().astype(np.int64), w.permute(0, 3, 1, 2).numpy(), 1)
    for dt in (torch.float64, torch.float32):
        assert np.array_equal(R.conv_acc(x, w, dt)[0].permute(2, 0, 1).numpy(), want)
    assert np.abs(want).max() > 2 ** 21


def test_yolo_ref_equals_oracle():
    g = torch.Generator().manual_seed(4)
    head = torch.randn(2, 36, 13, 20, generator=g) * 1.5     # NCHW, as the oracle takes it
    img_size = (13 * 16, 20 * 16)
    wio, wp = U.yolo_decode(head, img_size)
    io, p = R.yolo_ref(head.permute(0, 2, 3, 1), 6, 6, torch.tensor(U.ANCHORS, dtype=torch.float32), 16.0)
    assert torch.equal(p.float(), wp)
    assert ((io - wio.double()).norm() / io.norm()).item() <= 1e-6


def test_round_half_even_known_answer():
    """den = levels = 1 (w_bit 2, a_bit 1), alpha = 0.5, shift = 0: acc 1 -> v = 0.5 exactly -> code 0 (half up: 1),
    acc 3 -> clamped code 1; v = 0.5 is a possible tie by construction, so the GPU test asserts the value itself."""
    acc = torch.tensor([1, 3, 2, 0]).view(1, 1, 4, 1)
    codes, tie = R.codes_ref(acc, 1, torch.tensor([0.5]), torch.tensor([0.0]), 1, False)
    assert codes.flatten().tolist() == [0, 1, 1, 0] and tie.flatten().tolist() == [True, False, False, False]


def test_assert_codes_tie_proven():
    ref = torch.arange(4000).view(1, 10, 20, 20) % 16
    tie = torch.zeros_like(ref, dtype=torch.bool)
    tie[0, 0, 0, 1] = True
    got = ref.clone()
    got[0, 0, 0, 1] += 1
    R.assert_codes_tie_proven(got, ref, tie, 1e-3)
    got[0, 0, 0, 2] += 1
    with pytest.raises(AssertionError, match="outside possible ties"):
        R.assert_codes_tie_proven(got, ref, tie, 1e-3)
    got[0, 0, 0, 2] -= 1
    got[0, 0, 0, 1] += 1
    with pytest.raises(AssertionError, match="off by 2"):
        R.assert_codes_tie_proven(got, ref, tie, 1e-3)
    with pytest.raises(AssertionError, match="vacuous"):
        R.assert_codes_tie_proven(ref, ref, tie, 1e-4)


# ---- every GPU parametrisation: caps and spread on the reference alone ----------------------------------------------
def _spread(codes, levels):
    return len(torch.unique(codes)) >= min(8, levels + 1)


@pytest.mark.parametrize("a_bit", R.CONV0_ABITS)
def test_conv0_caps(a_bit):
    shares = {}
    sizes = R.CONV0_SIZES + [(R.conv0_walk_batch(R.NOMINAL_CUS, H, W), H, W) for H, W in R.CONV0_WALK_MAPS]
    for B, H, W in sizes:
        c = R.conv0_case(B, H, W, a_bit)
        shares[(B, H, W)] = R.tie_share(c.tie)
        assert R.tie_share(c.tie) <= R.CAP_CONV0, (B, H, W)
        assert _spread(c.codes, R.a_levels(a_bit)), (B, H, W)
    print("conv0 possible-tie shares", a_bit, {k: f"{v:.2e}" for k, v in shares.items()})


def test_conv0_walk_batches():
    for H, W in R.CONV0_WALK_MAPS:
        for cus in (R.NOMINAL_CUS, 304, 64):
            n = R.conv0_walk_batch(cus, H, W) * 9
            assert n >= 16 * cus and n % 8 != 0


@pytest.mark.parametrize("w_bit,a_bit", R.CONV_BITS)
def test_conv_caps(w_bit, a_bit):
    worst = 0.0
    for cin, ks, cout, mode, _ in R.CONV_CASES:
        for shape in R.CONV_MAPS[mode]:
            c = R.conv_case(cin, ks, cout, mode, shape, w_bit, a_bit)
            assert int(c.acc.abs().max()) < 2 ** 24
            if mode == "f32":
                continue
            worst = max(worst, R.tie_share(c.tie))
            assert R.tie_share(c.tie) <= R.CAP_INT_ACC, (cin, ks, cout, mode, shape)
            assert _spread(c.codes, c.levels), (cin, ks, cout, mode, shape)
    print("conv worst possible-tie share", (w_bit, a_bit), f"{worst:.2e}")


@pytest.mark.parametrize("cin,ks,cout,mode", R.CONV_WALK)
def test_conv_walk_caps(cin, ks, cout, mode):
    B, H, W = R.WALK_MAP
    ntiles = B * ((H + 15) // 16) * ((W + 15) // 16)
    assert ntiles > 2048 and ntiles % 8 != 0
    c = R.conv_case(cin, ks, cout, mode, R.WALK_MAP, 4, 4, torch.float32)
    print("conv walk possible-tie share", (cin, ks, cout, mode), f"{R.tie_share(c.tie):.2e}")
    assert R.tie_share(c.tie) <= R.CAP_INT_ACC and _spread(c.codes, 15)


@pytest.mark.parametrize("out_bit,sbits", R.CONV0_INT_BITS)
def test_conv0_int_inputs(out_bit, sbits):
    sizes = list(R.CONV0_SIZES)
    if (out_bit, sbits) == R.WALK_INT_BITS:
        sizes += [(R.conv0_walk_batch(R.NOMINAL_CUS, H, W), H, W) for H, W in R.CONV0_WALK_MAPS]
    for B, H, W in sizes:
        c = R.conv0_int_case(B, H, W, out_bit, sbits)
        assert (c.img == 0).any() and (c.img == 255).any()
        assert (c.inc < 0).any() and (c.inc > 0).any()
        assert R.product_overflows(c.acc, c.inc).any(), (B, H, W)
        assert _spread(c.codes, R.a_levels(out_bit)), (B, H, W, len(torch.unique(c.codes)))


@pytest.mark.parametrize("out_bit,sbits", R.CONV_INT_BITS)
def test_conv_int_inputs(out_bit, sbits):
    for cin, cout, pool, _ in R.CONV_INT_CASES:
        c = R.conv_int_case(cin, cout, pool, R.CONV_INT_MAP, out_bit, sbits)
        assert (c.inc < 0).any() and (c.inc > 0).any()
        assert int((c.acc * c.inc.to(torch.int64)).abs().max()) >= 2 ** 32, (cin, cout)
        assert _spread(c.codes, R.a_levels(out_bit)), (cin, cout, pool, len(torch.unique(c.codes)))


@pytest.mark.parametrize("cin,cout", R.CONV_INT_WALK)
def test_conv_int_walk_inputs(cin, cout):
    out_bit, sbits = R.WALK_INT_BITS
    c = R.conv_int_case(cin, cout, True, R.WALK_MAP, out_bit, sbits, torch.float32)
    assert (c.inc < 0).any() and (c.inc > 0).any()
    assert int((c.acc * c.inc.to(torch.int64)).abs().max()) >= 2 ** 32
    assert _spread(c.codes, R.a_levels(out_bit))


@pytest.mark.parametrize("mode", ["codes", "pool"])
def test_conv_max_acc_case(mode):
    c = R.conv_max_case(mode)
    assert int(c.acc.max()) == 576 * 127 * 127 and int(c.acc.min()) == -576 * 127 * 127
    assert R.tie_share(c.tie) <= R.CAP_INT_ACC and _spread(c.codes, c.levels)
    full = c.codes[:, 2:-2, 2:-2, :2]                        # the two full-scale channels: inside the code range,
    assert (full > 0).all() and (full < c.levels).all()      # and (unpooled) other codes on the border
    assert mode == "pool" or len(torch.unique(c.codes[..., :2])) >= 3


@pytest.mark.parametrize("w_bit", range(2, 9))
def test_weight_code_caps(w_bit):
    for name, w in R.weight_cases(w_bit).items():
        v, tie = R.weight_ratio_ties(w, w_bit)
        assert R.tie_share(tie) <= R.CAP_WEIGHT, (name, R.tie_share(tie))
        want = U.weight_codes(w, w_bit).to(torch.int64)
        assert torch.equal(want[~tie], torch.round(v).to(torch.int64)[~tie]), name   # the fp32 oracle, outside ties
        assert int(want.abs().max()) == R.w_levels(w_bit)


@pytest.mark.parametrize("case", R.TAIL_CASES)
def test_tail_inputs(case):
    B, H, W, w_bit, a_bit, hout, dec, gain = case
    B = R.NOMINAL_CUS + 44 if B is None else B
    c = R.tail_case(B, H, W, w_bit, a_bit, hout, gain)
    print("tail images without a possible tie", case, int(c.clean.sum()), "of", B)
    assert 2 * int(c.clean.sum()) >= B
    assert _spread(c.last, R.a_levels(a_bit))
    assert c.head.shape == (B, H, W, hout) and len(torch.unique(c.head)) >= min(8, c.head.numel() // 2)


def test_yolo_cases():
    counts = [B * ny * nx * na * no for B, ny, nx, na, no, _ in R.YOLO_CASES]
    assert max(counts) >= 2 * 256 * 16 * 256                   # every thread of the capped grid takes a second element
    assert any(pad for *_, pad in R.YOLO_CASES)
