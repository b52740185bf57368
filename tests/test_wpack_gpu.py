"""csrc/wpack.hip on the device: the kernel cases of tests/wpack_cases.py (as tests/test_wpack_emulated_cpu.py runs them on the shim),
the modules that take their packed parameters from it -- outputs and every parameter gradient with the family on and off, from the
same weights, with the deferred chunk sums poisoned until their flush --, `encode()` on its own, and the launches of a forward pass."""
import contextlib

import pytest
import torch

import wpack_cases as W

pytestmark = pytest.mark.gpu
LEVELS = W.LEVELS
S = sum(h * w for h, w in LEVELS)


def dev():
    return torch.device("cuda", 0)


def test_wpack_every_size_alignment_and_form_in_one_call_equals_cat_and_add():
    W.check_sizes_alignments_and_both_forms(dev())


def test_wpack_adjacent_row_blocks_of_one_tensor_leave_their_neighbours_alone():
    W.check_adjacent_blocks_of_one_tensor(dev())


def test_wpack_one_job_more_than_the_cap_takes_a_second_launch():
    W.check_one_job_more_than_the_cap(dev())


def test_wpack_bf16_sums_are_rounded_once():
    W.check_bf16_sums_round_once(dev())


def test_wpack_pack_sites_forward_and_the_views_of_its_backward():
    W.check_pack_sites_autograd(dev())


def test_wpack_level_positions_equal_the_framework_expression_and_padding_keeps_it():
    W.check_level_positions(dev())


# ---- the modules ---------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def committed(family_on):
    """The committed bf16 families with / without MDETR_PARAM_PACK; registered chunk sums hold NaN until their flush."""
    import bench
    from monodetr_amd import chunk_sums
    names = set(bench.COMMITTED_SWITCHES["bf16"]) - {"MDETR_PARAM_PACK"}
    bench.apply_switches(names | ({"MDETR_PARAM_PACK"} if family_on else set()))
    was = chunk_sums.POISON
    chunk_sums.POISON = True
    try:
        yield
    finally:
        chunk_sums.POISON = was
        bench.apply_switches(set())


def level_tensors():
    shapes = torch.tensor(LEVELS, dtype=torch.long, device=dev())
    return shapes, torch.cat((shapes.new_zeros((1,)), shapes.prod(1).cumsum(0)[:-1]))


def rand(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(torch.bfloat16).to(dev())


def both_ways(build, sites_of, run):
    """build() -> module (same seed, same weights both times); sites_of(module) -> the modules whose packed parameters are handed
    out when the family is on (as DepthAwareTransformer does); run(module) -> [outputs].  -> outputs and gradients, off and on."""
    from monodetr_amd import chunk_sums, wpack_ext
    from monodetr_amd.monodetr.depthaware_transformer import DepthAwareTransformer
    res = {}
    for on in (False, True):
        with committed(on):
            torch.manual_seed(11)
            module = build().to(torch.bfloat16).to(dev()).train()
            with torch.no_grad():
                for i, p in enumerate(module.parameters()):           # (the reference initialises several of these projections to zero)
                    p.copy_(rand(*p.shape, seed=100 + i, scale=0.05 if p.dim() > 1 else 0.5))
            if on:
                sites = [(m,) + m._pack_site() for m in sites_of(module)]
                packed = wpack_ext.pack_sites(sites)
                assert len(packed) == len(sites) > 0
                DepthAwareTransformer._hand_out(packed)
            outs = run(module)
            assert all("_packed_now" not in m.__dict__ for m in module.modules())         # every handed pair was taken
            with chunk_sums.deferred(params=list(module.parameters())) as d:
                assert d.reason is None
                torch.autograd.backward(outs, [rand(*o.shape, seed=7 + k) for k, o in enumerate(outs)])
            res[on] = ([o.detach() for o in outs], {n: p.grad for n, p in module.named_parameters()})
    (out_off, g_off), (out_on, g_on) = res[False], res[True]
    for a, b in zip(out_off, out_on):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    assert set(g_off) == set(g_on)
    for n in g_off:
        assert (g_off[n] is None) == (g_on[n] is None), n
        if g_off[n] is not None:
            assert torch.isfinite(g_on[n].float()).all(), n
            assert torch.equal(g_off[n], g_on[n]), n
    return g_on


def test_wpack_deformable_attention_module_matches_its_own_packing():
    from monodetr_amd.monodetr.ops.modules import MSDeformAttn
    shapes, starts = level_tensors()
    query, value = rand(2, 7, 256, seed=1).requires_grad_(True), rand(2, S, 256, seed=2).requires_grad_(True)
    ref = torch.rand(2, 7, len(LEVELS), 2, generator=torch.Generator().manual_seed(3)).to(dev())
    g = both_ways(lambda: MSDeformAttn(256, len(LEVELS), 8, 4), lambda m: [m], lambda m: [m(query, ref, value, shapes, starts)])
    assert all(g[n] is not None for n in ("sampling_offsets.weight", "sampling_offsets.bias", "attention_weights.weight", "attention_weights.bias"))


def test_wpack_encoder_layer_matches_its_own_packing():
    from monodetr_amd.monodetr.depthaware_transformer import VisualEncoder, VisualEncoderLayer
    shapes, starts = level_tensors()
    src, pos = rand(2, S, 256, seed=1).requires_grad_(True), rand(2, S, 256, seed=2)
    ref = VisualEncoder.get_reference_points(LEVELS, torch.ones(2, len(LEVELS), 2, device=dev()), dev())
    both_ways(lambda: VisualEncoderLayer(256, 64, 0.0, "relu", len(LEVELS), 8, 4), lambda m: [m.self_attn],
              lambda m: [m(src, pos, ref, shapes, starts)])


def test_wpack_decoder_layer_with_two_query_groups_matches_its_own_packing():
    from monodetr_amd.monodetr.depthaware_transformer import DepthAwareDecoderLayer
    shapes, starts = level_tensors()
    tgt, qpos = rand(2, 6, 256, seed=1).requires_grad_(True), rand(2, 6, 256, seed=2)
    memory, depth = rand(2, S, 256, seed=3).requires_grad_(True), rand(5, 2, 256, seed=4)
    ref = (0.2 + 0.6 * torch.rand(2, 6, 1, 6, generator=torch.Generator().manual_seed(5))).expand(-1, -1, len(LEVELS), -1).to(dev())
    g = both_ways(lambda: DepthAwareDecoderLayer(256, 64, 0.0, "relu", len(LEVELS), 8, 4, group_num=2), lambda m: [m, m.cross_attn],
                  lambda m: [m(tgt, qpos, ref, memory, shapes, starts, None, depth, None, 2)])
    for n in ("sa_qcontent_proj", "sa_qpos_proj", "sa_kcontent_proj", "sa_kpos_proj"):
        assert g[n + ".weight"] is not None and g[n + ".bias"] is not None
    assert torch.equal(g["sa_qcontent_proj.weight"], g["sa_qpos_proj.weight"]) and torch.equal(g["sa_kcontent_proj.bias"], g["sa_kpos_proj.bias"])


def test_wpack_encode_alone_leaves_the_decoder_sites_without_gradient():
    """`encode()` without the decoder behind it (the graph of `bench.py --config 2`): memory and gradients equal the family-off run,
    the sources of the decoder's packed tensors get no gradient, nothing raises; a following whole-module call packs afresh."""
    from monodetr_amd import chunk_sums
    from monodetr_amd.monodetr.depthaware_transformer import DepthAwareTransformer
    from monodetr_amd.utils.misc import NestedTensor
    res = {}
    for on in (False, True):
        with committed(on):
            torch.manual_seed(5)
            model = DepthAwareTransformer(256, 8, 2, 1, 64, 0.0, "relu", False, len(LEVELS), 4, 4, group_num=2).to(torch.bfloat16).to(dev()).train()
            with torch.no_grad():
                for i, p in enumerate(model.parameters()):
                    p.copy_(rand(*p.shape, seed=300 + i, scale=0.05 if p.dim() > 1 else 0.5))
            srcs = [rand(2, 256, h, w, seed=20 + l).requires_grad_(True) for l, (h, w) in enumerate(LEVELS)]
            levels = W.sine_levels(dev(), 256, 2)
            masks = [x.mask for _, x in levels]
            pos = [pe(x).to(torch.bfloat16) for pe, x in levels]
            for p in pos:
                p._mdetr_sine_const = True                    # (as backbone.Joiner marks the casts it keeps)
            for it in range(2):
                model.zero_grad(set_to_none=True)
                memory = model.encode(srcs, masks, pos)[0]
                assert ("_decoder_packs" in model.__dict__ and len(model.__dict__["_decoder_packs"]) == 2) == on
                with chunk_sums.deferred(params=list(model.parameters())) as d:
                    assert d.reason is None
                    memory.backward(rand(*memory.shape, seed=9))
            res[on] = (memory.detach(), {n: p.grad for n, p in model.named_parameters()})
    (m_off, g_off), (m_on, g_on) = res[False], res[True]
    assert torch.isfinite(m_on.float()).all() and torch.equal(m_off, m_on)
    for n in g_off:
        assert (g_off[n] is None) == (g_on[n] is None), n
        if n.startswith("decoder.") or n.startswith("reference_points."):
            assert g_on[n] is None, n
        elif g_on[n] is not None:
            assert torch.isfinite(g_on[n].float()).all() and torch.equal(g_off[n], g_on[n]), n
    assert g_on["level_embed"] is not None and g_on["encoder.layers.1.self_attn.attention_weights.weight"] is not None


# ---- the whole step ------------------------------------------------------------------------------------------------------------
PARAM_SHAPES = {(256, 256), (128, 256), (256,), (128,)}


def forward_launches(step):
    """(kernel launches, CatArrayBatchedCopy launches, concatenations of parameter-sized operands, kernel names) of one eager forward
    pass + criterion: the kernels from the profiler, the operands of every aten::cat from a dispatch mode around one more pass."""
    from torch.profiler import ProfilerActivity, profile
    from torch.utils._python_dispatch import TorchDispatchMode
    param_cats = []

    class CatLog(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if func is torch.ops.aten.cat.default:
                operands = {tuple(t.shape) for t in args[0]}
                if operands <= PARAM_SHAPES:
                    param_cats.append(sorted(operands))
            return func(*args, **(kwargs or {}))

    with CatLog():
        step._forward(step.inputs)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step._forward(step.inputs)
        torch.cuda.synchronize()
    launches = cats = 0
    names = set()
    for e in prof.events():
        if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower():
            launches += 1
            cats += "CatArrayBatchedCopy" in e.name
            names.add(e.name)
    return launches, cats, param_cats, names


def test_wpack_forward_pass_drops_the_launches_that_follow_from_the_code():
    """One eager forward pass of bench.py's step at batch 1 under the profiler, family off and on.  Off: 12 `cat` of the six
    deformable-attention modules, 12 `add` + 6 `cat` of the three decoder layers, 4 `add` + 1 `cat` of the level positions (no cast:
    encoding, embedding and result share a dtype).  On: one `pack_params` and one `level_pos` launch instead: 35 - 2 launches less,
    19 concatenation kernels less, and no concatenation of parameter-sized operands left."""
    import bench
    seen = {}
    try:
        for on in (False, True):
            names = set(bench.COMMITTED_SWITCHES["bf16"]) - {"MDETR_PARAM_PACK"} | ({"MDETR_PARAM_PACK"} if on else set())
            step = bench.TrainStep(dev(), 1, "bf16", size=(384, 1280), switches=names)
            seen[on] = forward_launches(step)
            del step
    finally:
        bench.apply_switches(set())
    (n_off, cat_off, pc_off, k_off), (n_on, cat_on, pc_on, k_on) = seen[False], seen[True]
    print("forward launches: off %d on %d; CatArrayBatchedCopy: off %d on %d; parameter concatenations: off %d on %d"
          % (n_off, n_on, cat_off, cat_on, len(pc_off), len(pc_on)))
    assert len(pc_off) == 18 and pc_on == [], (pc_off, pc_on)
    assert any("pack_params_kernel" in k for k in k_on) and any("level_pos_kernel" in k for k in k_on)
    assert not any("pack_params_kernel" in k or "level_pos_kernel" in k for k in k_off)
    assert cat_off - cat_on == 19, (cat_off, cat_on)
    assert n_off - n_on == 33, (n_off, n_on)


def test_wpack_training_step_matches_the_step_without_it():
    """The committed bf16 list with and without MDETR_PARAM_PACK, chunk sums poisoned until their flush: the kernels of the step see
    the same operand bits, so the loss trajectories differ only by what the step's floating-point atomics leave (the bound of
    test_training_step_with_the_fold_kernel_matches_default, 1e-3 relative)."""
    import bench
    from model_init import disable_dropout_
    traj = {}
    for on in (False, True):
        with committed(on):
            names = set(bench.COMMITTED_SWITCHES["bf16"]) - {"MDETR_PARAM_PACK"} | ({"MDETR_PARAM_PACK"} if on else set())
            step = bench.TrainStep(dev(), 2, "bf16", size=(96, 320), switches=names)
            disable_dropout_(step.raw_model)
            traj[on] = [float(step()) for _ in range(3)]
            del step
    print("loss trajectories: off %s on %s" % (traj[False], traj[True]))
    for a, b in zip(traj[False], traj[True]):
        assert a == a and abs(a - b) <= 1e-3 * abs(a), traj
