"""Head-geometry prune groups without a GPU: tests/prune_heads_ref.py's permutation, the host's unit-to-row expansion
and table filling (quantized_vit_amd.qat_prune.prune_tables), vit_head_prune_groups' declaration, the constructor's new
rejections, compress_pruned_heads as tensor surgery on CPU modules, the exports, and the condition on the schedule
test's inputs: the reference run prunes a head and leaves one in each block."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn as nn

import prune_heads_common as C
import prune_heads_ref as P
from prune_step_ref import PruneF64, PruneHyper

GEOMS = [(2, 4), (3, 4), (2, 64), (3, 64)]


@pytest.mark.parametrize("H,hd", GEOMS)
def test_permutation_round_trips_and_a_unit_is_the_heads_rows(H, hd):
    from quantized_vit_amd.qat_prune import unit_rows_of, units_view
    K = 5
    w = torch.arange(3 * H * hd * K, dtype=torch.float32).reshape(3 * H * hd, K)
    b = torch.arange(3 * H * hd, dtype=torch.float32)
    for x, tail in ((w, (K,)), (b, ())):
        for form in (x, x.numpy()):
            u = P.to_units(form, H, hd)
            assert tuple(u.shape) == (H, 3 * hd * (K if tail else 1))
            back = P.from_units(u, H, hd, tail)
            assert tuple(back.shape) == tuple(x.shape) and (np.asarray(back) == x.numpy()).all()
        for h in range(H):
            rows = P.unit_rows(h, H, hd)
            # head h as the forward's reshape(B, N, 3, H, hd) reads the projection's columns
            want = np.arange(3 * H * hd).reshape(3, H, hd)[:, h].reshape(-1)
            assert (rows == want).all()
            assert (unit_rows_of([h], H, 3, hd) == rows).all()
            assert torch.equal(P.to_units(x, H, hd)[h], x[rows].reshape(-1))
        assert torch.equal(units_view(x, H, 3, hd), P.to_units(x, H, hd))
    order = [H - 1, 0]
    assert (unit_rows_of(order, H, 3, hd) == np.concatenate([P.unit_rows(h, H, hd) for h in order])).all()
    assert (unit_rows_of([3, 1], 7) == [3, 1]).all()   # one row per unit: the rows themselves, in the given order


def _states(groups):
    from quantized_vit_amd.qat_prune import _GroupState
    out = [_GroupState(g) for g in groups]
    for g in out:
        g.prunable = True
    return out


def _i64(a):
    """A descriptor array as the int64 words that reach the device, one row per descriptor."""
    return a.view(np.int64).reshape(len(a), a.dtype.itemsize // 8)


@pytest.mark.parametrize("H,hd", GEOMS)
def test_table_filling(H, hd):
    from quantized_vit_amd import PruneGroup, _lib
    from quantized_vit_amd.qat_prune import prune_tables
    K = 3
    head = PruneGroup("h", None, [torch.zeros(3 * H * hd, K), torch.zeros(3 * H * hd)], sections=3, unit_rows=hd)
    basic = PruneGroup("b", None, [torch.zeros(6, K)])
    gs = _states([basic, head])
    assert (gs[0].rows, gs[0].num_groups, gs[0].basic) == (6, 6, True)
    assert (gs[1].rows, gs[1].num_groups, gs[1].basic) == (3 * H * hd, H, False)
    gs[0].active, gs[0].pruned = [4, 1], [0]
    gs[1].active, gs[1].pruned = [H - 1], [0] if H > 2 else []
    grow = np.zeros(2, dtype=_lib.PRUNE_GROUP_DTYPE)
    t = prune_tables(gs, [0, 1], True, grow)
    assert all(t[k].dtype == _lib.PRUNE_ITEM_DTYPE for k in ("items", "units", "red"))
    assert t["items"]["row"][:6].tolist() == list(range(6)) and t["red"]["row"][:2].tolist() == [4, 1]
    assert grow["rows"].tolist() == [6, 3 * H * hd] and grow["joint"].tolist() == [1, 1]
    assert grow["red_begin"].tolist() == [0, 2] and grow["red_count"].tolist() == [2, 3 * hd]
    grow = _i64(grow)
    t = {k: v if k == "joint" else _i64(v) for k, v in t.items()}   # the packed words, as the tables were before

    def split(a):
        return a[:, 0] & 0xffffffff, a[:, 0] >> 32, a[:, 1] & 0xffffffff, a[:, 1] >> 32
    grp, row, state, link = split(t["items"])
    assert len(grp) == 6 + 3 * H * hd
    assert (grp[:6] == 0).all() and (row[:6] == np.arange(6)).all() and (link[:6] == 0).all()
    assert state[:6].tolist() == [2, 1, 0, 0, 1, 0]
    assert (grp[6:] == 1).all() and (row[6:] == np.arange(3 * H * hd)).all()
    unit_state = np.zeros(H, dtype=np.int64)
    unit_state[gs[1].active], unit_state[gs[1].pruned] = _lib.PRUNE_REDUNDANT, _lib.PRUNE_PRUNED
    for h in range(H):
        rows = P.unit_rows(h, H, hd)
        assert (link[6:][rows] == h).all() and (state[6:][rows] == unit_state[h]).all()
    # the units: the BASIC group's rows, then the heads, each pointing at its group's row 0 in items
    grp, row, state, link = split(t["units"])
    assert grp.tolist() == [0] * 6 + [1] * H and row.tolist() == list(range(6)) + list(range(H))
    assert link.tolist() == [0] * 6 + [6] * H and state[6:].tolist() == unit_state.tolist()
    # the redundant list: a group's rows contiguous, a unit's rows in the fold's order
    grp, row, state, link = split(t["red"])
    assert grp.tolist() == [0, 0] + [1] * (3 * hd) and row[:2].tolist() == [4, 1]
    assert (row[2:] == P.unit_rows(H - 1, H, hd)).all() and (link[2:] == H - 1).all() and (state == 1).all()
    assert t["joint"] == [0, 1]
    assert grow[0, 4] == 6 | (1 << 32) and grow[0, 5] == 0 | (2 << 32)
    assert grow[1, 4] == 3 * H * hd | (1 << 32) and grow[1, 5] == 2 | ((3 * hd) << 32)
    # one-row groups alone: the tables of before (no link anywhere, no unit table)
    gs = _states([basic])
    gs[0].active = [2]
    t = prune_tables(gs, [0], False, np.zeros(1, dtype=_lib.PRUNE_GROUP_DTYPE))
    t = {k: v if k == "joint" else _i64(v) for k, v in t.items()}
    assert (t["items"][:, 1] >> 32 == 0).all() and t["units"].shape == (0, 2) and t["red"].tolist() == [[2 << 32, 1]]


def _cpu_vit(seed=0):
    from quantized_vit_amd.vit_model import VisionTransformer
    torch.manual_seed(seed)
    return VisionTransformer(representation_size=None, **C.VIT).eval()


def test_vit_head_prune_groups_declares_the_forwards_heads():
    from quantized_vit_amd import vit_head_prune_groups
    model = _cpu_vit()
    groups = vit_head_prune_groups(model)
    assert [g.name for g in groups] == ["blocks.0.attn", "blocks.1.attn"]
    for g, blk in zip(groups, model.blocks):
        assert g.layer is blk.attn.qkv and (g.sections, g.unit_rows) == (3, 64)
        assert len(g.members) == 2 and g.members[0] is blk.attn.qkv.weight and g.members[1] is blk.attn.qkv.bias
    model.blocks[1].attn.qkv.bias = None
    assert [len(g.members) for g in vit_head_prune_groups(model)] == [2, 1]


def test_constructor_rejections_of_the_new_geometry():
    from quantized_vit_amd import PruneGroup
    from quantized_vit_amd.qat_prune import _check_prune_groups
    net = C.make_net(torch.device("cpu"))
    ok = PruneGroup("g", net.l0, [net.l0.weight, net.l0.bias], sections=3, unit_rows=4)
    _check_prune_groups([ok])
    for kw in (dict(sections=0), dict(unit_rows=0), dict(sections=-3), dict(unit_rows=2.0), dict(sections=True)):
        with pytest.raises(ValueError, match="sections|unit_rows"):
            _check_prune_groups([PruneGroup("g", net.l0, [net.l0.weight], **kw)])
    with pytest.raises(ValueError, match=r"sections \* units \* unit_rows"):   # 36 rows are no multiple of 3 * 5
        _check_prune_groups([PruneGroup("g", net.l0, [net.l0.weight], sections=3, unit_rows=5)])
    with pytest.raises(ValueError, match=r"sections \* units \* unit_rows"):   # 33 rows, sections = 2
        _check_prune_groups([PruneGroup("g", net.l2, [net.l2.weight, net.l2.bias], sections=2)])
    with pytest.raises(ValueError, match="shape"):   # members of different row counts: no common number of units
        _check_prune_groups([PruneGroup("g", net.l0, [net.l0.weight, net.l2.bias], sections=3)])


def _zero_heads(model, sets):
    with torch.no_grad():
        for blk, heads in zip(model.blocks, sets):
            rows = P.rows_of_units(heads, C.VIT_HEADS, C.VIT_HD)
            blk.attn.qkv.weight[rows] = 0
            blk.attn.qkv.bias[rows] = 0


@pytest.mark.parametrize("order", ["heads_then_mlp", "mlp_then_heads"])
def test_compress_pruned_heads_shapes_on_cpu_modules(order):
    from quantized_vit_amd import compress_pruned_heads, compress_pruned_mlp, convert
    model = _cpu_vit()
    _zero_heads(model, [[2], [0, 1, 3]])
    with torch.no_grad():
        model.blocks[0].mlp.fc1.weight[:100] = 0
        model.blocks[0].mlp.fc1.bias[:100] = 0
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        want = model(x)
    proj_cols = [model.blocks[i].attn.proj.weight.detach().clone() for i in range(2)]
    steps = [compress_pruned_heads, compress_pruned_mlp]
    for f in (steps if order == "heads_then_mlp" else steps[::-1]):
        assert f(model) is model
    dim, hd = C.VIT["embed_dim"], C.VIT_HD
    for i, (blk, left) in enumerate(zip(model.blocks, (3, 1))):
        a = blk.attn
        assert (a.num_heads, a.head_dim, a.scale) == (left, hd, hd ** -0.5)
        assert tuple(a.qkv.weight.shape) == (3 * left * hd, dim) and tuple(a.qkv.bias.shape) == (3 * left * hd,)
        assert tuple(a.proj.weight.shape) == (dim, left * hd) and tuple(a.proj.bias.shape) == (dim,)
        kept = [h for h in range(4) if h not in ([2], [0, 1, 3])[i]]
        cols = np.concatenate([np.arange(h * hd, (h + 1) * hd) for h in kept])
        assert torch.equal(a.proj.weight, proj_cols[i][:, cols])
        assert a.qkv.weight.abs().sum(dim=1).min() > 0
    assert model.blocks[0].mlp.fc1.out_features == C.VIT_HIDDEN - 100
    with torch.no_grad():
        got = model(x)
    # fp32 modules on the CPU: a head of zeros adds exact zeros, the proj sum loses only those terms
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-6)
    again = convert.vit_from_state_dict(model.state_dict())
    assert [b.attn.num_heads for b in again.blocks] == [3, 1]
    assert [b.mlp.fc1.out_features for b in again.blocks] == [C.VIT_HIDDEN - 100, C.VIT_HIDDEN]
    with torch.no_grad():
        assert torch.equal(again(x), got)
    assert compress_pruned_heads(model) is model and [b.attn.num_heads for b in model.blocks] == [3, 1]   # idempotent


def test_compress_pruned_heads_refuses_a_block_without_heads():
    from quantized_vit_amd import compress_pruned_heads
    model = _cpu_vit()
    _zero_heads(model, [[], [0, 1, 2, 3]])
    with pytest.raises(ValueError, match="no head left"):
        compress_pruned_heads(model)
    model = _cpu_vit()
    model.blocks[0].attn.num_heads = 3   # a model whose attribute and tensors disagree is refused, not guessed at
    with pytest.raises(ValueError, match="outputs"):
        compress_pruned_heads(model)


def test_a_head_with_a_nonzero_bias_entry_stays():
    from quantized_vit_amd import compress_pruned_heads
    model = _cpu_vit()
    _zero_heads(model, [[1], [1]])
    with torch.no_grad():
        model.blocks[1].attn.qkv.bias[2 * 4 * 64 + 64 + 5] = 0.5   # head 1's v section
    compress_pruned_heads(model)
    assert [b.attn.num_heads for b in model.blocks] == [3, 4]


def test_exports():
    from quantized_vit_amd import _lib, build
    import quantized_vit_amd as Q
    header = (Path(build.INCLUDE) / "qvit_hip.h").read_text()
    assert "qvit_prune_scores_fold" in _lib.EXPORTED_SYMBOLS
    assert re.search(r"\bint\s+qvit_prune_scores_fold\(([^;]*)\);", header)
    assert "qvit_prune_scores_fold" in header.split("*/")[0]
    assert "int32_t group, row, state, link;" in header and "sections, unit_rows; }" in header
    assert "scores_fold:" in header   # the documented order of its checks
    for name in ("vit_head_prune_groups", "compress_pruned_heads"):
        assert name in Q.__all__ and callable(getattr(Q, name))


def test_the_declared_vit_groups_are_the_references_and_its_run_prunes_heads_under_the_cosine_criterion():
    """vit_head_prune_groups + vit_mlp_prune_groups declare, in order, the groups the GPU schedule test hands to the
    reference (names, members, units), and the condition on that test's inputs holds: the reference run prunes a head
    and leaves one in each block. The reference's default criteria cannot take a head of this model: a head's
    magnitude and Taylor terms are those of 49 344 elements against an MLP unit's 257, and its overall score is 0.18 ..
    0.23 where no MLP unit exceeds 0.023 (printed below; three gradient seeds, none takes a head). The cosine criterion
    alone ranks heads among the MLP units; with it every head is selected and the group_divisible refinement gives one
    back per block."""
    from quantized_vit_amd import vit_head_prune_groups, vit_mlp_prune_groups
    from quantized_vit_amd.qat_prune import _GroupState
    from test_gpu_prune_step import NSTEPS, SCHEDULE
    model = C.head_vit(torch.device("cpu"))
    names = {id(p): n for n, p in model.named_parameters()}
    declared = [_GroupState(g) for g in vit_head_prune_groups(model) + vit_mlp_prune_groups(model)]
    start = {n: p.detach().clone() for n, p in model.named_parameters()}
    for criteria, seeds in ((None, (C.GRAD_SEED, 600, 700)), (C.COSINE, (C.GRAD_SEED,))):
        for seed in seeds:
            ref = PruneF64(P.permute({k: v.numpy() for k, v in start.items()}, C.VIT_SPECS),
                           PruneHyper(**SCHEDULE, criteria=criteria), C.vit_ref_groups())
            assert [(g.name, g.members, g.num_groups) for g in ref.groups] == \
                [(g.name, [names[id(p)] for p in g.members], g.num_groups) for g in declared]
            for s in range(NSTEPS):
                ref.step(P.permute({k: v.numpy() for k, v in C.vit_grads(start, s, seed).items()}, C.VIT_SPECS))
            heads = [ref.pruned_rows()[f"blocks.{i}.attn"] for i in range(2)]
            print("criteria", criteria, "seed", seed, "heads pruned", heads, "last scores: heads",
                  np.round(ref.last_scores[:8], 3), "largest MLP unit", float(ref.last_scores[8:].max()))
            assert sum(len(v) for v in ref.pruned_rows().values()) == ref.target
            if criteria is not None:
                assert any(heads) and all(len(h) < C.VIT_HEADS for h in heads)
            else:
                assert not any(heads) and ref.last_scores[:8].min() > 5 * ref.last_scores[8:].max()
