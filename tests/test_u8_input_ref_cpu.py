"""The reference of the uint8 image input judged on its own (tests/u8_input_ref.py), without a GPU: the value table is
ToTensor + Normalize element for element, the parameter sets are free of rounding ties, and the case table tells a
swapped layout and a transposed table from the correct result."""
import pytest
import torch

import conv_geometry_ref as G
import u8_input_ref as U


def _all_bytes_image(C):
    """[1, C, 16, 32] uint8 holding every byte value in every channel, in a different order per channel."""
    g = torch.Generator().manual_seed(3)
    chans = [torch.cat([torch.randperm(256, generator=g), torch.randperm(256, generator=g)]) for _ in range(C)]
    return torch.stack(chans).to(torch.uint8).view(1, C, 16, 32)


@pytest.mark.parametrize("mean,std", [U.HALF, U.IMAGENET, ((0.1, 0.9, 0.5, 0.25), (0.3, 1.7, 0.5, 2.0))])
def test_value_table_is_totensor_then_normalize(mean, std):
    C = len(mean)
    img = _all_bytes_image(C)
    m, s = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
    want = (img[0].float().div(255) - m[:, None, None]) / s[:, None, None]
    table = U.value_table(mean, std)
    assert table.dtype == torch.float32 and tuple(table.shape) == (C, 256)
    got = U.value_image(img, table)[0]
    assert torch.equal(got, want)
    for c in range(C):                       # and entry by entry
        assert torch.equal(table[c][img[0, c].reshape(-1).long()], want[c].reshape(-1))


@pytest.mark.parametrize("ps", U.PARAM_SETS, ids=U.PARAM_IDS)
def test_parameter_sets_are_tie_free(ps):
    """float32 and float64 codes agree on all 768 table values; every unsaturated value is at least
    MIN_TIE_DISTANCE of a step from a rounding tie in float64."""
    table = U.value_table(ps.mean, ps.std)
    assert table.numel() == 768
    c32, c64 = U.codes(table, ps, torch.float32), U.codes(table, ps, torch.float64)
    assert torch.equal(c32.double(), c64)
    assert int(c64.abs().max()) == ps.L                       # the set saturates, at the level it names
    dist = U.tie_distance(table, ps)
    assert dist.numel() > 256
    print(f"{ps.id}: min tie distance {float(dist.min()):.3e} steps over {dist.numel()} unsaturated values")
    assert float(dist.min()) >= U.MIN_TIE_DISTANCE


def test_tie_set_sits_on_a_tie():
    """Why TIE_SET is kept out of the oracle comparisons: bytes 0 and 255 are 3.5 steps of 2 / 7, and miss the tie
    only by the rounding of d = float32(2 / 7): one float32 ulp of the quotient, which an approximate division can
    land on either side of."""
    ps = U.TIE_SET
    table = U.value_table(ps.mean, ps.std)
    assert float(table[0, 255]) == 1.0 and float(table[0, 0]) == -1.0
    assert float(U.tie_distance(table, ps).min()) < 2.0 ** -22


def test_case_table():
    ids = U.U8_CASE_IDS
    assert len(set(ids)) == len(ids) and set(G.CASE_IDS) < set(ids)
    by = {c.id: c for c in U.U8_CASES}
    assert by["U1"].xshape == (2, 3, 16, 48) and by["U1"].H * by["U1"].W == 768
    assert by["U2"].W == 52 and by["U3"].shifted and by["U4"].C == 4 and by["U5"].k == (14, 14)
    arms = {(i, lay): U.takes_vector_arm(by[i], lay) for i in ("U1", "U2", "U3", "U4", "U5")
            for lay in (U.NCHW, U.NHWC)}
    assert arms == {("U1", 0): True, ("U1", 1): True, ("U2", 0): False, ("U2", 1): False, ("U3", 0): False,
                    ("U3", 1): False, ("U4", 0): True, ("U4", 1): False, ("U5", 0): False, ("U5", 1): False}
    img = U.make_image(by["U1"])
    for c in range(3):                                        # every byte value in every channel
        assert torch.unique(img[0, c]).numel() == 256
    assert not torch.equal(img[0, 0], img[0, 1])


@pytest.mark.parametrize("case", U.U8_CASES, ids=U.U8_CASE_IDS)
def test_reference_is_the_gather(case):
    """ref_rows equals the kernel's index arithmetic (conv_geometry_ref.gather_codes) on the per-pixel codes."""
    ps = U.PARAM_SETS[2]
    img = U.make_image(case)
    per_pixel = U.oracle_code_image(ps)(img)
    assert torch.equal(U.ref_rows(img, case, U.oracle_code_image(ps)), G.gather_codes(per_pixel, case))


@pytest.mark.parametrize("case", U.U8_CASES, ids=U.U8_CASE_IDS)
def test_table_discriminates(case):
    """A kernel that reads NHWC bytes as NCHW, or indexes the table [v][c], gives other rows (C > 1)."""
    ps = U.PARAM_SETS[2]                                      # per-channel mean and std: the channels' tables differ
    img = U.make_image(case)
    C = case.C
    good = U.ref_rows(img, case, U.oracle_code_image(ps))
    if C == 1:
        assert torch.equal(U.nhwc_bytes_as_nchw(img), img)
        return
    swapped = U.ref_rows(U.nhwc_bytes_as_nchw(img), case, U.oracle_code_image(ps))
    assert not torch.equal(swapped, good)
    table = U.codes(U.value_table(*ps.channels(C)), ps)       # [C][256]
    flat = table.reshape(-1)

    def transposed(img_u8):                                   # entry v*C + c of the [c][v] bytes
        c_idx = torch.arange(C).view(1, C, 1, 1)
        return flat[img_u8.long() * C + c_idx]
    assert not torch.equal(U.ref_rows(img, case, transposed), good)
