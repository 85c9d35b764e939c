"""CPU checks of the plan lifecycle helpers (tests/plan_lifecycle_ref.py): the twin builder, the mutation table's
coverage of the plan key, the tie cap of the chosen seeds on the oracle alone, and negative controls of the comparers.
No device: layers are built on the CPU, where they hold parameters but run nothing."""
import pytest
import torch

import plan_lifecycle_ref as P

CPU_MUTATIONS = [m for m in P.MUTATIONS if m != "sgd_step"]   # the SGD entry runs a forward: device only


def _state(layer):
    return {k: v.detach().clone() for k, v in layer.state_dict().items()}


@pytest.mark.parametrize("name", list(P.LAYERS))
def test_twin_has_the_state_and_shares_nothing(name):
    layer = P.build_layer(name, "cpu")
    if name == "conv":
        layer.set_uint8_input((0.5, 0.4, 0.3), 0.25)
    layer.train()
    twin = P.fresh_twin(layer)
    assert type(twin) is type(layer) and twin.training
    assert twin.quant_type == layer.quant_type and twin.quant_mode == layer.quant_mode
    assert not P.unequal_routes(_state(twin), _state(layer))
    assert getattr(twin, "uint8_input", None) == getattr(layer, "uint8_input", None)
    mine = {p.untyped_storage().data_ptr() for p in layer.parameters()}
    assert not mine & {p.untyped_storage().data_ptr() for p in twin.parameters()}
    with torch.no_grad():
        twin.weight.mul_(2.0)
    assert P.unequal_routes(_state(twin), _state(layer)) == ["weight"]


def test_mutation_table_touches_every_key_tensor():
    """Every tensor QuantizeMixin._plan_key reads (_quant_param_tensors) is named by at least one table entry, and an
    entry changes exactly the tensors it names."""
    layer = P.build_layer("qkv", "cpu")
    names = {id(p): n for n, p in layer.named_parameters()}
    key_names = [names[id(p)] for p in layer._quant_param_tensors()]
    assert key_names == P.PARAM_NAMES
    touched = set().union(*(set(t) for t, _ in P.MUTATIONS.values()))
    assert set(key_names) <= touched
    for mutation in CPU_MUTATIONS:
        layer = P.build_layer("qkv", "cpu")
        before = _state(layer)
        P.MUTATIONS[mutation][1](layer)
        assert not layer.training
        assert sorted(P.unequal_routes(_state(layer), before)) == sorted(P.MUTATIONS[mutation][0]), mutation


def _oracle_alone(layer):
    """The oracle's codes beside the same quantizer with correctly rounded log / exp (oracle.ties.cr_codes: the
    device's careful path): how many codes two faithful implementations give differently on these weights."""
    from oracle.ties import cr_codes
    own, q = P.oracle_weight_codes(layer)
    w = layer.weight.detach().reshape(own.shape)
    return P.codes_tie_stats(w, cr_codes(w, q["q_type"], q["d"], q["q_m"], q["t"]), own, q)


@pytest.mark.parametrize("name", list(P.LAYERS))
def test_tie_cap_holds_on_the_oracle_alone(name):
    """On the chosen seeds, in the initial state and after every mutation, the oracle differs from its correctly
    rounded restatement on at most TIE_SHARE_CAP of the weight codes, and tie_check proves each difference a tie: the
    GPU comparison at that cap is neither vacuous nor out of reach."""
    for mutation in [None] + CPU_MUTATIONS:
        layer = P.build_layer(name, "cpu")
        if mutation is not None:
            if not all(hasattr(layer, n) for n in P.MUTATIONS[mutation][0]):
                continue
            P.MUTATIONS[mutation][1](layer)
        st = _oracle_alone(layer)
        assert st["flips"] <= P.TIE_SHARE_CAP * st["total"] and st["non_ties"] == 0, (mutation, st)


@pytest.mark.parametrize("name", ["qkv", "lin"])
def test_tie_cap_holds_across_the_storage_classes(name):
    layer = P.build_layer(name, "cpu")
    for move, edit, _ in P.CLASS_MOVES:
        edit(layer)
        st = _oracle_alone(layer)
        assert st["flips"] <= P.TIE_SHARE_CAP * st["total"] and st["non_ties"] == 0, (move, st)
        if move in ("w16", "w24", "fp32", "back_w4"):
            assert st["flips"] == 0, (move, st)      # redrawn tie-free at the new quantizer


def test_class_moves_reach_the_levels_they_name():
    from quantized_vit_amd import _lib
    from quantized_vit_amd.quant_layers import saturation_level
    layer = P.build_layer("qkv", "cpu")
    f = lambda n: float(getattr(layer, n).detach())
    seen = []
    for move, edit, expect in P.CLASS_MOVES:
        edit(layer)
        lw = saturation_level(_lib.QT_NONLINEAR, f("d_quant_wt"), f("q_m_wt"), f("t_quant_wt"))
        la = saturation_level(_lib.QT_NONLINEAR, f("d_quant_act"), f("q_m_act"), f("t_quant_act"))
        seen.append((move, lw, la))
    assert seen == [("w8", 127, 127), ("w4", 7, 127), ("act_wide", 7, 1000), ("act_int8", 7, 127),
                    ("w16", 32000, 127), ("w24", 60000, 127), ("fp32", 100000, 127), ("back_w4", 7, 127)]


def test_a_twin_from_before_a_mutation_is_reported_unequal():
    """Negative control of unequal_routes on what the CPU can compute of a layer: its state and the oracle's codes."""
    for mutation in CPU_MUTATIONS:
        layer = P.build_layer("qkv", "cpu")
        before = P.fresh_twin(layer)
        P.MUTATIONS[mutation][1](layer)
        view = lambda l: dict(_state(l), codes=P.oracle_weight_codes(l)[0])
        bad = P.unequal_routes(view(before), view(layer))
        assert bool(bad) == bool(P.MUTATIONS[mutation][0]), (mutation, bad)
        assert not P.unequal_routes(view(P.fresh_twin(layer)), view(layer))
    a = {"y": torch.zeros(3)}
    assert P.unequal_routes(a, {"y": torch.zeros(3, dtype=torch.float64)}) == ["y"]      # dtype
    assert P.unequal_routes(a, {"y": torch.zeros(4)}) == ["y"]                           # shape
    assert P.unequal_routes(a, {"y": torch.tensor([0.0, 0.0, 1e-45])}) == ["y"]          # one denormal bit
    assert P.unequal_routes(a, {}) == ["y"] and P.unequal_routes({}, a) == ["y"]         # a missing route


def test_codes_proven_rejects_what_it_should():
    ok = dict(flips=3, non_ties=0, cr_explained=1, total=49152)
    assert P.codes_proven(ok)
    assert not P.codes_proven(dict(ok, non_ties=1, cr_explained=3))      # a difference that is no proven tie
    assert not P.codes_proven(dict(ok, flips=50, cr_explained=50))       # more than TIE_SHARE_CAP of the codes
    layer = P.build_layer("qkv", "cpu")
    own, q = P.oracle_weight_codes(layer)
    w = layer.weight.detach().reshape(own.shape)
    wrong = own.clone()
    wrong[5, 7] += 1                                                     # tie-free weights: one wrong code is no tie
    assert not P.codes_proven(P.codes_tie_stats(w, wrong, own, q))


def test_a_mixed_set_of_routes_is_reported_mixed():
    old = {"forward": torch.tensor([1.0]), "packed": torch.tensor([1.0]), "bits": torch.tensor([4])}
    new = {"forward": torch.tensor([2.0]), "packed": torch.tensor([2.0]), "bits": torch.tensor([4])}
    all_old = P.classify_routes(dict(old), old, new)
    assert all_old == {"forward": "old", "packed": "old", "bits": "both"} and not P.is_mixed(all_old)
    all_new = P.classify_routes(dict(new), old, new)
    assert all_new == {"forward": "new", "packed": "new", "bits": "both"} and not P.is_mixed(all_new)
    mixed = P.classify_routes({"forward": old["forward"], "packed": new["packed"], "bits": old["bits"]}, old, new)
    assert mixed == {"forward": "old", "packed": "new", "bits": "both"} and P.is_mixed(mixed)
    stray = P.classify_routes({"forward": torch.tensor([3.0]), "packed": old["packed"]}, old, new)
    assert stray["forward"] == "neither" and P.is_mixed(stray)


# ---- the plan's own decoders, against the kernels' layout formulas restated element by element ------------------
def _perm_row(rho):   # quant_kernels.hip perm_row
    return (rho & ~63) | (((rho >> 2) & 3) << 4) | (((rho >> 4) & 3) << 2) | (rho & 3)


def _pack_ref(codes, w4: bool, npad: int, kpad: int) -> torch.Tensor:
    """qvit_pack_weight's image of integer codes, byte by byte (quant_kernels.hip: packed_offset, pack_weight_kernel)."""
    n, k = codes.shape
    rowb = 32 if w4 else 64
    out = bytearray(npad * kpad // 2 if w4 else npad * kpad)
    for rho in range(npad):
        row = _perm_row(rho)
        for k0 in range(0, kpad, 8):
            kc = [int(codes[row, k0 + i]) if row < n and k0 + i < k else 0 for i in range(8)]
            nb, r, st, kk = rho >> 8, rho & 255, k0 >> 6, k0 & 63
            tile, c = (nb * (kpad >> 6) + st) * (256 * rowb), kk >> 4
            if w4:
                off = tile + r * rowb + 8 * (c ^ (((r >> 3) & 1) << 1)) + ((kk & 15) >> 1)
                for b in range(4):
                    out[off + b] = (kc[b] & 0xF) | ((kc[b + 4] & 0xF) << 4)
            else:
                off = tile + r * rowb + 16 * (c ^ (((r >> 2) & 1) << 1)) + (kk & 15)
                for b in range(8):
                    out[off + b] = kc[b] & 0xFF
    return torch.tensor(list(out), dtype=torch.uint8)


@pytest.mark.parametrize("w4", [True, False])
def test_unpack_codes_inverts_the_pack_layout(w4):
    from quantized_vit_amd import _lib
    from quantized_vit_amd.quant_layers import unpack_codes
    n, k, npad, kpad = 300, 130, 512, 256     # two row blocks, four k-stages, padding on both axes
    lo, hi = (-8, 8) if w4 else (-128, 128)
    codes = torch.randint(lo, hi, (n, k), generator=torch.Generator().manual_seed(0))
    got = unpack_codes(_pack_ref(codes, w4, npad, kpad), _lib.W4 if w4 else _lib.W8, npad, kpad)
    assert torch.equal(got[:n, :k], codes.float())
    assert not got[n:].any() and not got[:, k:].any()


def test_unpack_codes_sums_the_wide_digits():
    from quantized_vit_amd import _lib
    from quantized_vit_amd.quant_layers import unpack_codes
    codes = torch.tensor([[70000, -70000, 32639, -32768, 255, -129, 0, 4000000]])
    npad, kpad = 256, 64
    digits, r = [], codes.clone()
    for _ in range(3):                           # balanced base-256 digits (_lib.pack_weight_wide)
        d = torch.remainder(r + 128, 256) - 128
        digits.append(d)
        r = (r - d) // 256
    assert not r.any()
    image = torch.cat([_pack_ref(d, False, npad, kpad) for d in reversed(digits)])
    assert torch.equal(unpack_codes(image, _lib.W24, npad, kpad)[:1, :8], codes.float())


@pytest.mark.parametrize("w8r", [False, True])
def test_unpack_wreg_inverts_the_register_images(w8r):
    """pack_w4r_kernel / pack_w8r_kernel (gemm_w4a8.hip) restated fragment by fragment, then unpack_wreg."""
    from quantized_vit_amd import _lib
    from quantized_vit_amd.quant_layers import unpack_wreg
    npad, kpad = 256, 128                        # two chunks of 8 KiB
    src = torch.randint(0, 256, (npad * kpad // 2,), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    dst = torch.zeros(npad * kpad if w8r else npad * kpad // 2, dtype=torch.uint8)
    for u in range(src.numel() // 8):
        c, w, ln, r = u >> 10, (u >> 8) & 3, (u >> 2) & 63, u & 3
        lfr, lfq = ln & 15, ln >> 4
        row = 64 * w + 16 * r + lfr
        so = c * 8192 + row * 32 + ((lfq ^ (((lfr >> 3) & 1) << 1)) << 3)
        frag = src[so:so + 8]
        if w8r:
            x, y = frag[:4], frag[4:]
            do = c * 16384 + w * 4096 + ln * 64 + r * 16
            dst[do:do + 16] = torch.cat([(x << 4) & 0xF0, x & 0xF0, (y << 4) & 0xF0, y & 0xF0])
        else:
            do = c * 8192 + w * 2048 + ln * 32 + r * 8
            dst[do:do + 8] = frag
    assert torch.equal(unpack_wreg(dst, _lib.W8R if w8r else _lib.W4R, npad, kpad), src)
