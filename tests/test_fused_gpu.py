"""GPU tests of the optional kernel families (fused criterion, flat AdamW, residual LayerNorm, MSDA prologue, bf16-native
MSDA, convolution / FFN tails, library GEMM + ReLU epilogue, 3x3 convolution, token GEMM), the input pipeline kernel and the
evaluation kernels: each family against the framework operators / the default path it replaces.  First GPU run: round 2
(profiles/r02a_pytest_fused_gpu.log, 56 of 57 green; the 57th was this file's own end-to-end configuration).  A family
may be listed in bench.COMMITTED_SWITCHES only while its tests here are green."""
import os

import pytest
import torch
from conftest import tune  # noqa: E402

pytestmark = [pytest.mark.gpu]


def test_fused_adamw_kernel_matches_foreach_adamw():
    from monodetr_amd.helpers.optimizer_helper import AdamW, FusedAdamW

    def make():
        torch.manual_seed(5)
        w4 = torch.nn.Parameter(torch.randn(64, 32, 3, 3, device="cuda").contiguous(memory_format=torch.channels_last))
        b1 = torch.nn.Parameter(torch.randn(77, device="cuda"))
        wl = torch.nn.Parameter(torch.randn(333, 170, device="cuda").to(torch.bfloat16))
        bl = torch.nn.Parameter(torch.randn(333, device="cuda").to(torch.bfloat16))
        big = torch.nn.Parameter(torch.randn(2048, 1024, device="cuda"))
        groups = [{'params': [b1, bl], 'weight_decay': 0}, {'params': [w4, wl, big], 'weight_decay': 1e-2}]
        return [w4, b1, wl, bl, big], groups

    pa, ga = make()
    pb, gb = make()
    oa, ob = AdamW(ga, lr=1e-3), FusedAdamW(gb, lr=1e-3)
    for step in range(5):
        gen = torch.Generator(device="cuda").manual_seed(100 + step)
        for x, y in zip(pa, pb):
            g = torch.randn(x.shape, generator=gen, device="cuda")
            if x.dim() == 4:
                g = g.contiguous(memory_format=torch.channels_last)
            x.grad, y.grad = g.to(x.dtype), g.to(y.dtype).clone()
        oa.step(); ob.step()
    assert ob._flat is not None and len(ob._flat[1]) == 4
    for x, y in zip(pa, pb):
        assert x.stride() == y.stride()
        tol = 1e-6 if x.dtype == torch.float32 else 1e-2
        assert (x.detach().float() - y.detach().float()).abs().max() <= tol * max(1.0, x.detach().float().abs().max().item())
    assert (oa.state[pa[2]]['master'] - ob.state[pb[2]]['master']).abs().max() < 1e-5
    # capturable: device-resident step size gives the same result
    pc, gc = make()
    oc = FusedAdamW(gc, lr=1e-3, capturable=True)
    for step in range(5):
        gen = torch.Generator(device="cuda").manual_seed(100 + step)
        for z in pc:
            g = torch.randn(z.shape, generator=gen, device="cuda")
            if z.dim() == 4:
                g = g.contiguous(memory_format=torch.channels_last)
            z.grad = g.to(z.dtype)
        oc.step()
    for y, z in zip(pb, pc):
        assert (y.detach().float() - z.detach().float()).abs().max() <= 1e-5 * max(1.0, y.detach().float().abs().max().item())


def test_fused_adamw_vs_recorded_reference_steps():
    """adamw.hip on the GPU against six recorded steps of the REFERENCE's own optimizer (lib/helpers/optimizer_helper.py:
    69-129; tests/golden/optimizer_adamw.npz recorded in fp64 by tests/golden/make_optimizer_golden.py): fp32 arithmetic
    against the fp64 recording, 1e-6 of the parameter scale; a parameter that receives its first gradient at step 2 included."""
    from conftest import load_golden
    from optimizer_problem import make_grads, make_model
    from monodetr_amd.helpers.optimizer_helper import FusedAdamW, build_optimizer
    g = load_golden("optimizer_adamw")
    shadow, model = make_model(), make_model().float().cuda()
    opt = build_optimizer({'type': 'adamw', 'lr': 2e-4, 'weight_decay': 1e-4, 'fused': True}, model)
    assert isinstance(opt, FusedAdamW)
    for step in range(6):
        make_grads(shadow, step)
        for ps, p in zip(shadow.parameters(), model.parameters()):
            p.grad = None if ps.grad is None else ps.grad.float().cuda()
        opt.step()
        if step in (0, 5):
            for n, p in model.named_parameters():
                ref = torch.as_tensor(g["step%d/%s" % (step, n)])
                assert (p.detach().cpu().double() - ref).abs().max() <= 1e-6 * max(1.0, ref.abs().max().item()), (step, n)


def test_training_step_with_fused_adamw_matches_default():
    """Three full training iterations (bf16 body, dropout off): the loss trajectory with the fused
    optimizer follows the default one."""
    import bench
    from model_init import disable_dropout_
    dev = torch.device("cuda", 0)
    traj = {}
    for fused in (False, True):
        os.environ["MDETR_FUSED_ADAMW"] = "1" if fused else "0"
        try:
            step = bench.TrainStep(dev, 2, "bf16", size=(96, 320))
        finally:
            os.environ.pop("MDETR_FUSED_ADAMW", None)
        disable_dropout_(step.raw_model)
        traj[fused] = [float(step()) for _ in range(3)]
    assert type(step.optimizer).__name__ == "FusedAdamW"
    for a, b in zip(traj[False], traj[True]):
        assert abs(a - b) <= 2e-2 * abs(a), traj


def test_fused_pair_losses_kernel_matches_the_criterion():
    """csrc/pair_losses.hip (launch glue, reductions, last-block finalisation, workspace self-cleaning)
    against the PyTorch criterion on the GPU: all loss entries and the gradients of the five prediction
    tensors, twice in a row (the second call runs on the workspace the first one left behind)."""
    from test_fused_losses_cpu import _problem
    from model_init import load_cfg
    from monodetr_amd.monodetr import build_monodetr
    torch.manual_seed(0)
    _, criterion = build_monodetr(load_cfg())
    criterion.train().cuda()
    for (L, B, Q, K, G, seed) in ((3, 8, 550, 50, 11, 1), (3, 4, 110, 7, 11, 0)):
        preds, gt = _problem(L, B, Q, K, G, seed)
        preds = {k: v.cuda() for k, v in preds.items()}
        gt = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in gt.items()}
        criterion.group_num = G
        outputs = {k: v[-1] for k, v in preds.items()}
        outputs['pred_depth_map_logits'] = torch.randn(B, 81, 6, 20, device="cuda")
        outputs['aux_outputs'] = [{k: v[i] for k, v in preds.items()} for i in range(L - 1)]

        def run(fused):
            criterion.fused_pair_losses = fused
            leaves = {k: v.clone().requires_grad_(True) for k, v in preds.items()}
            losses = criterion(dict(outputs, _levels=leaves), gt)
            criterion.weighted_total(losses).backward()
            return losses, {k: v.grad for k, v in leaves.items()}

        ref_losses, ref_grads = run(False)
        for _ in range(2):
            got_losses, got_grads = run(True)
            for k in ref_losses:
                a, b = float(ref_losses[k]), float(got_losses[k])
                assert abs(a - b) <= 1e-4 * max(1.0, abs(a)), (k, a, b)
            for k in ref_grads:
                assert (ref_grads[k] - got_grads[k]).abs().max().item() <= 1e-4 * ref_grads[k].abs().max().item() + 1e-9, k


@pytest.mark.parametrize("layout", ["contiguous", "channels_last"])
def test_fused_ddn_loss_kernel_matches_the_pytorch_ddn_loss(layout):
    """csrc/ddn_loss.hip against DDNLoss on the GPU at the training shape (8 x 81 x 24 x 80, 50 slots):
    value and gradient, twice in a row (workspace self-cleaning)."""
    from monodetr_amd.ddn_loss_ext import fused_ddn_loss
    from monodetr_amd.monodetr.depth_predictor.ddn_loss import DDNLoss
    from monodetr_amd.utils import box_ops
    g = torch.Generator().manual_seed(3)
    B, C, H, W, K = 8, 81, 24, 80, 50
    logits = torch.randn(B, C, H, W, generator=g).cuda()
    if layout == "channels_last":
        logits = logits.contiguous(memory_format=torch.channels_last)
    boxes = torch.cat((torch.rand(B, K, 2, generator=g), 0.05 + 0.4 * torch.rand(B, K, 2, generator=g)), -1).cuda()
    depth = (2 + 60 * torch.rand(B, K, generator=g)).cuda()
    num = torch.randint(0, 9, (B,), generator=g)
    valid = (torch.arange(K)[None, :] < num[:, None]).cuda()
    ref_mod = DDNLoss()
    za = logits.clone().requires_grad_(True)
    xyxy = box_ops.box_cxcywh_to_xyxy(torch.stack((boxes[..., 0] * W, boxes[..., 1] * H, boxes[..., 2] * W, boxes[..., 3] * H), -1))
    xyxy = torch.where(valid[..., None], xyxy, torch.zeros_like(xyxy))
    ref = ref_mod(za, xyxy.reshape(-1, 4), K, depth.reshape(-1), valid=valid.reshape(-1))
    ref.backward()
    for _ in range(2):
        zb = logits.clone().requires_grad_(True)
        got = fused_ddn_loss(zb, boxes, depth, valid, ref_mod.alpha, ref_mod.balancer.fg_weight, ref_mod.balancer.bg_weight)
        got.backward()
        assert abs(float(ref) - float(got)) <= 1e-5 * abs(float(ref))
        assert (za.grad - zb.grad).abs().max() <= 1e-4 * za.grad.abs().max()


def test_fused_cost_solver_kernel_matches_scipy():
    """csrc/lsa.hip with the cost evaluated in the kernel against scipy on the PyTorch cost matrix (equal
    total cost per problem; assignments are permutations of the group's queries)."""
    import numpy as np
    from scipy.optimize import linear_sum_assignment
    from test_fused_losses_cpu import _problem
    from model_init import load_cfg
    from monodetr_amd.lsa_ext import batched_assignment_fused
    from monodetr_amd.monodetr import build_monodetr
    _, crit = build_monodetr(load_cfg())
    m = crit.matcher
    for (L, B, Q, K, G, seed) in ((3, 8, 550, 50, 11, 0), (2, 3, 110, 7, 11, 1), (1, 2, 64, 64, 1, 2)):
        preds, gt = _problem(L, B, Q, K, G, seed)
        cost = m.cost_padded(preds['pred_logits'], preds['pred_boxes'], gt).double().numpy()
        gtc = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in gt.items()}
        got = batched_assignment_fused(preds['pred_logits'].cuda(), preds['pred_boxes'].cuda(), gtc, G,
                                       (m.cost_class, m.cost_bbox, m.cost_3dcenter, m.cost_giou)).cpu().numpy()
        n = Q // G
        for l in range(L):
            for b in range(B):
                k = int(gt['num'][b])
                for g in range(G):
                    a = got[l, b, g]
                    assert (a[k:] == -1).all()
                    if k:
                        sub = cost[l, b, g * n:(g + 1) * n, :k]
                        r, c = linear_sum_assignment(sub)
                        mine = a[:k] - g * n
                        assert len(set(mine.tolist())) == k and mine.min() >= 0 and mine.max() < n
                        assert abs(sub[r, c].sum() - sub[mine, np.arange(k)].sum()) <= 1e-5 * max(1.0, abs(sub[r, c].sum()))


def test_training_step_with_fused_criterion_matches_default():
    """Three full training iterations (bf16 body, dropout off) with MDETR_FUSED_LOSSES=1 (fused matching cost,
    pair losses, depth-map loss): the loss trajectory follows the default one."""
    import bench
    from model_init import disable_dropout_
    dev = torch.device("cuda", 0)
    traj = {}
    for fused in (False, True):
        os.environ["MDETR_FUSED_LOSSES"] = "1" if fused else "0"
        try:
            step = bench.TrainStep(dev, 2, "bf16", size=(96, 320))
        finally:
            os.environ.pop("MDETR_FUSED_LOSSES", None)
        assert step.criterion.fused_pair_losses == fused and step.criterion.matcher.fused_cost == fused
        disable_dropout_(step.raw_model)
        traj[fused] = [float(step()) for _ in range(3)]
    for a, b in zip(traj[False], traj[True]):
        assert abs(a - b) <= 2e-2 * abs(a), traj


def test_token_linear_layer_with_the_token_gemm_matches_default():
    """token_linear forward + input gradient through csrc/tgemm.hip (MDETR_TGEMM) against the library path."""
    import importlib
    from monodetr_amd.monodetr import linear
    torch.manual_seed(9)
    x = torch.randn(8, 10200, 256, device="cuda").to(torch.bfloat16).requires_grad_(True)
    w = (torch.randn(256, 256, device="cuda") / 16).to(torch.bfloat16).requires_grad_(True)
    b = torch.randn(256, device="cuda").to(torch.bfloat16).requires_grad_(True)
    g = torch.randn(8, 10200, 256, device="cuda").to(torch.bfloat16)
    for relu in (False, True):                                      # relu=True: ReLU in the kernel's epilogue
        res = {}
        for flag in (False, True):
            linear._TGEMM = flag
            try:
                y = linear.token_linear(x, w, b, relu=relu)
                res[flag] = (y.detach().float(),) + tuple(t.float() for t in torch.autograd.grad(y, (x, w, b), g))
            finally:
                linear._TGEMM = False
        for a, c in zip(res[False], res[True]):
            assert ((a - c).norm() / a.norm()).item() < 6e-3


@pytest.mark.parametrize("R,Lq,dtype", [(2, 10200, torch.float32), (2, 10200, torch.bfloat16), (6, 550, torch.float32),
                                        (6, 550, torch.bfloat16)])
def test_msda_prologue_kernel_matches_module_formulas(R, Lq, dtype):
    """csrc/msda_prologue.hip at the encoder (R = 2) and decoder (R = 6, broadcast reference points) shapes against
    the module's PyTorch formulation evaluated in fp32, values and gradients."""
    from test_msda_prologue_cpu import torch_prologue
    from monodetr_amd.msda_prologue_ext import msda_prologue
    B, M, L, P = 8, 8, 4, 4
    g = torch.Generator().manual_seed(R)
    shapes = torch.tensor([(48, 160), (24, 80), (12, 40), (6, 20)], dtype=torch.int64).cuda()
    offsets = (torch.randn(B, Lq, M, L, P, 2, generator=g) * 3).to(dtype).cuda().requires_grad_(True)
    logits = torch.randn(B, Lq, M, L * P, generator=g).to(dtype).cuda().requires_grad_(True)
    if R == 6:
        base = torch.rand(B, Lq, R, generator=g).to(dtype).cuda().requires_grad_(True)
        ref = base[:, :, None].expand(-1, -1, L, -1)
    else:
        base = torch.rand(B, Lq, L, R, generator=g).to(dtype).cuda().requires_grad_(True)
        ref = base
    g_loc = torch.randn(B, Lq, M, L, P, 2, generator=g).cuda()
    g_att = torch.randn(B, Lq, M, L, P, generator=g).cuda()
    loc_r, att_r = torch_prologue(offsets, logits, ref, shapes, P)
    ref_grads = torch.autograd.grad([loc_r, att_r], [offsets, logits, base], [g_loc, g_att])
    loc, att = msda_prologue(offsets, logits, ref, shapes)
    got_grads = torch.autograd.grad([loc, att], [offsets, logits, base], [g_loc, g_att])
    assert (loc - loc_r).abs().max() < 1e-5 and (att - att_r).abs().max() < 1e-6
    tol = 1e-4 if dtype == torch.float32 else 2e-2
    for a, b in zip(ref_grads, got_grads):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert (a.float() - b.float()).abs().max() <= tol * max(1.0, a.float().abs().max().item())


def _msda_problem(B, Lq, M, shapes, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    sh = torch.tensor(shapes, dtype=torch.int64, device="cuda")
    start = torch.cat([sh.new_zeros(1), (sh[:, 0] * sh[:, 1]).cumsum(0)[:-1]])
    S = int((sh[:, 0] * sh[:, 1]).sum())
    Lq = S if Lq is None else Lq
    value = torch.randn(B, S, M, 32, generator=g, device="cuda").to(torch.bfloat16)
    loc = torch.rand(B, Lq, M, 4, 4, 2, generator=g, device="cuda") * 1.3 - 0.15      # some samples leave the map
    attn = torch.softmax(torch.randn(B, Lq, M, 16, generator=g, device="cuda"), -1).view(B, Lq, M, 4, 4)
    grad_out = torch.randn(B, Lq, M * 32, generator=g, device="cuda").to(torch.bfloat16)
    return value, sh, start, loc, attn, grad_out


@pytest.mark.parametrize("B,Lq,M,shapes", [
    (2, None, 8, [(12, 40), (6, 20), (3, 10), (2, 5)]),         # self-attention: tile-privatised grad_value
    (2, 50, 8, [(12, 40), (6, 20), (3, 10), (2, 5)]),           # decoder-like cross attention: atomics
    (8, None, 8, [(48, 160), (24, 80), (12, 40), (6, 20)]),     # the encoder shape of the benchmark
    (1, 3, 1, [(1, 1), (2, 3), (1, 7), (5, 1)]),                # degenerate maps, ragged tail
])
def test_msda_bf16_kernels_match_the_fp32_kernels_on_rounded_inputs(B, Lq, M, shapes):
    """The mixed-precision operator computes exactly what the fp32 operator computes on the widened bf16 tensors;
    the only differences are the final rounding of `out` to bf16 and the fp32 summation order."""
    from monodetr_amd import msda_ext
    value, sh, start, loc, attn, grad_out = _msda_problem(B, Lq, M, shapes, 3)
    out = msda_ext.ms_deform_attn_forward_bf16(value, sh, start, loc, attn)
    ref = msda_ext.ms_deform_attn_forward(value.float(), sh, start, loc, attn, 64)
    assert out.dtype == torch.bfloat16 and out.shape == ref.shape
    assert torch.equal(out, ref.to(torch.bfloat16)) or (out.float() - ref).abs().max() <= 2 ** -8 * ref.abs().max()
    gv, gl, ga = msda_ext.ms_deform_attn_backward_bf16(value, sh, start, loc, attn, grad_out)
    rv, rl, ra = msda_ext.ms_deform_attn_backward(value.float(), sh, start, loc, attn, grad_out.float(), 64)
    for got, want in ((gv, rv), (gl, rl), (ga, ra)):
        assert got.dtype == torch.float32 and got.shape == want.shape
        assert (got - want).abs().max() <= 1e-3 * max(1.0, want.abs().max().item())


def test_msda_function_with_native_bf16_matches_the_widening_path(monkeypatch):
    from monodetr_amd.monodetr.ops.functions import ms_deform_attn_func as F
    value, sh, start, loc, attn, grad_out = _msda_problem(2, None, 8, [(12, 40), (6, 20), (3, 10), (2, 5)], 4)
    res = {}
    for native in (False, True):
        monkeypatch.setattr(F, "_NATIVE_BF16", native)
        v = value.clone().requires_grad_(True)
        l = loc.to(torch.bfloat16).requires_grad_(True)
        a = attn.to(torch.bfloat16).requires_grad_(True)
        out = F.MSDeformAttnFunction.apply(v, sh, start, l, a, 64)
        out.backward(grad_out)
        res[native] = (out.detach(), v.grad, l.grad, a.grad)
    for x, y in zip(res[False], res[True]):
        assert x.dtype == y.dtype == torch.bfloat16
        assert (x.float() - y.float()).abs().max() <= 2 ** -7 * max(1.0, x.float().abs().max().item())


def test_training_step_with_bf16_msda_matches_default(monkeypatch):
    import bench
    from model_init import disable_dropout_
    from monodetr_amd.monodetr.ops.functions import ms_deform_attn_func as F
    dev = torch.device("cuda", 0)
    traj = {}
    for native in (False, True):
        monkeypatch.setattr(F, "_NATIVE_BF16", native)
        step = bench.TrainStep(dev, 2, "bf16", size=(96, 320))
        disable_dropout_(step.raw_model)
        traj[native] = [float(step()) for _ in range(3)]
    for a, b in zip(traj[False], traj[True]):
        assert abs(a - b) <= 2e-2 * abs(a), traj


# ---- input pipeline on the device ----------------------------------------------------------------
def _kitti_batch(n, seed, distort=True):
    import numpy as np
    import kitti_synth
    from monodetr_amd import kitti_prep_ext as prep
    from oracle import kitti_pipeline as okp
    rs = np.random.RandomState(seed)
    images, want = [], []
    for k in range(n):
        w, h = kitti_synth.SIZES[(seed + k) % 4]
        img = kitti_synth.synth_image(rs, w, h)
        np.random.seed(1000 * seed + k)
        d = np.zeros(1, dtype=prep.DESCRIPTOR)
        d['width'], d['height'], d['perm'] = w, h, prep.IDENTITY_PERM
        src = img
        if distort:
            from monodetr_amd.datasets.kitti.kitti_dataset import draw_photometric
            state = np.random.get_state()
            draw_photometric(d[0])
            np.random.set_state(state)
            src = okp.apply_photometric(img, okp.draw_photometric())
        flip, center, crop_size, _ = okp.draw_geometry(np.array([w, h]), scale=0.4, shift=0.1)
        if flip:
            d['flags'] |= prep.FLIP
        _, inv = okp.affine_pair(center, crop_size)
        d['inv'] = inv.reshape(-1)
        images.append({'pixels': img, 'descriptor': d})
        want.append(okp.warp_and_normalise(src, flip, inv))
    return images, np.stack(want)


@pytest.mark.parametrize("n,distort", [(1, False), (3, True), (8, True)])
def test_kitti_preprocess_kernel_is_bit_identical_to_the_reference_chain(n, distort):
    import numpy as np
    from monodetr_amd import kitti_prep_ext as prep
    from monodetr_amd.helpers.dataloader_helper import pack_images
    images, want = _kitti_batch(n, 11 + n, distort)
    packed, _ = pack_images(images)
    dev = packed.cuda()
    head = n * prep.DESCRIPTOR.itemsize
    out = prep.preprocess_batch(dev[head:], dev[:head])
    assert out.shape == (n, 3, 384, 1280)
    assert np.array_equal(out.cpu().numpy(), want)                      # bit-exact, float32
    bf = prep.preprocess_batch(dev[head:], dev[:head], dtype=torch.bfloat16)
    assert torch.equal(bf, out.to(torch.bfloat16))


def test_device_loader_yields_the_reference_loop_tuple(tmp_path):
    import numpy as np
    import kitti_synth
    from monodetr_amd.helpers.dataloader_helper import build_dataloader
    from oracle import kitti_pipeline as okp
    from PIL import Image
    root = str(tmp_path)
    ids = kitti_synth.make_tree(root, n_images=5, seed=9)
    cfg = {'type': 'KITTI', 'root_dir': root, 'aug_pd': True, 'aug_crop': True, 'train_split': 'train', 'test_split': 'val',
           'batch_size': 2, 'scale': 0.05, 'shift': 0.05, 'writelist': ['Car']}
    train, val = build_dataloader(cfg, workers=2)
    seen = 0
    for inputs, calibs, targets, info in val:                            # 3 batches (2, 2, 1), prefetch one ahead
        assert inputs.is_cuda and inputs.shape[1:] == (3, 384, 1280) and calibs.shape[1:] == (3, 4)
        for b, img_id in enumerate(info['img_id'].tolist()):
            img = np.array(Image.open('%s/training/image_2/%06d.png' % (root, img_id)))
            size = np.array([img.shape[1], img.shape[0]])
            _, inv = okp.affine_pair(size / 2, size)
            assert np.array_equal(inputs[b].cpu().numpy(), okp.warp_and_normalise(img, False, inv))
            seen += 1
    assert seen == 5
    n = sum(x.shape[0] for x, _, _, _ in train)                          # augmented, shuffled: runs and is finite
    assert n == 5 and all(torch.isfinite(x).all() for x, _, _, _ in train)


# ---- KITTI evaluation on the device ---------------------------------------------------------------
def test_rotated_overlap_kernels_match_the_oracle_on_the_gpu():
    import numpy as np
    from monodetr_amd.datasets.kitti.kitti_eval_python import rotate_iou
    from oracle import kitti_eval as oke
    rs = np.random.RandomState(5)
    frames_b, frames_q = [], []
    for f in range(7):
        n, k = [(5, 9), (0, 3), (12, 1), (3, 0), (8, 8), (1, 1), (20, 17)][f]
        mk = lambda m: np.stack([rs.uniform(-4, 4, m), rs.uniform(8, 16, m), rs.uniform(1.4, 4.5, m), rs.uniform(1.4, 4.5, m), rs.uniform(-3.2, 3.2, m)], 1)
        frames_b.append(mk(n)); frames_q.append(mk(k))
    frames_q[5] = frames_b[5].copy()                                    # identical boxes
    for crit in (-1, 0, 1, 2):
        got = rotate_iou.segmented_rotate_iou(frames_b, frames_q, crit)
        for b, q, o in zip(frames_b, frames_q, got):
            assert o.shape == (len(b), len(q)) and o.dtype == np.float32
            assert np.array_equal(o, oke.rotate_iou(b.astype(np.float32), q.astype(np.float32), crit))      # float32, same operations
    b7 = [np.concatenate([b[:, :1], rs.uniform(1.2, 2, (len(b), 1)), b[:, 1:2], b[:, 2:3], rs.uniform(1.3, 2, (len(b), 1)), b[:, 3:]], 1) for b in frames_b]
    q7 = [np.concatenate([q[:, :1], rs.uniform(1.2, 2, (len(q), 1)), q[:, 1:2], q[:, 2:3], rs.uniform(1.3, 2, (len(q), 1)), q[:, 3:]], 1) for q in frames_q]
    for crit in (-1, 0, 1):
        got = rotate_iou.segmented_box3d_overlap(b7, q7, crit)
        for b, q, o in zip(b7, q7, got):
            assert np.array_equal(o, oke.d3_box_overlap(b, q, crit).reshape(len(b), len(q)))
    one = rotate_iou.rotate_iou_gpu_eval(frames_b[6], frames_q[6])
    assert one.dtype == np.float64 and np.array_equal(one.astype(np.float32), got_first(frames_b[6], frames_q[6]))


def got_first(b, q):
    from oracle import kitti_eval as oke
    return oke.rotate_iou(b.astype('float32'), q.astype('float32'), -1)


def test_official_evaluation_on_the_gpu_matches_the_recorded_reference_report(tmp_path):
    import numpy as np
    import kitti_synth
    import kitti_synth_dets
    from monodetr_amd.datasets.kitti.kitti_eval_python import eval as kitti_eval
    from monodetr_amd.datasets.kitti.kitti_eval_python import kitti_common
    root = str(tmp_path)
    ids = kitti_synth.make_tree(root, n_images=40, seed=21, images=False, occ_choices=[0, 0, 0, 1, 2, 3])
    kitti_synth_dets.make_results(root, ids, os.path.join(root, 'results'), seed=3)
    g = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'kitti_eval.npz'))
    dt = kitti_common.get_label_annos(os.path.join(root, 'results'))
    gt = kitti_common.get_label_annos(os.path.join(root, 'training', 'label_2'), [int(i) for i in ids])
    for cls in (0, 1, 2):
        text, ret, moderate = kitti_eval.get_official_eval_result(gt, dt, cls)
        assert text == str(g['cls%d_text' % cls])
        assert abs(moderate - float(g['cls%d_ap3d_r40_moderate' % cls])) < 1e-12


# ---- the whole pipeline: loader -> training -> checkpoint -> inference -> result files -> official evaluation --------
def test_train_val_entry_point_end_to_end(tmp_path, monkeypatch):
    import yaml
    import kitti_synth
    from model_init import MODEL_CFG
    from monodetr_amd.tools import train_val
    monkeypatch.chdir(tmp_path)
    root = str(tmp_path / 'kitti')
    ids = kitti_synth.make_tree(root, n_images=12, seed=5, occ_choices=[0, 0, 1])
    cfg = {
        'random_seed': 444, 'model_name': 'monodetr',
        'dataset': {'type': 'KITTI', 'root_dir': root, 'train_split': 'train', 'test_split': 'val', 'batch_size': 2, 'use_3d_center': True,
                    'writelist': ['Car'], 'aug_pd': True, 'aug_crop': True, 'random_flip': 0.5, 'random_crop': 0.5, 'scale': 0.05,
                    'shift': 0.05, 'depth_scale': 'normal'},
        'model': dict(MODEL_CFG, device='cuda'),
        'optimizer': {'type': 'adamw', 'lr': 2e-4, 'weight_decay': 1e-4},
        'lr_scheduler': {'type': 'step', 'warmup': False, 'decay_rate': 0.1, 'decay_list': [125, 165]},
        'trainer': {'max_epoch': 2, 'gpu_ids': '0', 'save_frequency': 1, 'save_path': 'outputs/', 'save_all': True, 'use_dn': False,
                    'precision': 'bf16'},
        'tester': {'type': 'KITTI', 'mode': 'single', 'checkpoint': 2, 'threshold': 0.0, 'topk': 50},
    }
    path = str(tmp_path / 'cfg.yaml')
    yaml.safe_dump(cfg, open(path, 'w'))
    from monodetr_amd import group_norm_ext, kernel_families
    try:
        trainer = train_val.main(['--config', path])
        assert group_norm_ext.ENABLED                                   # the entry point trains with the committed kernel families
        # ... and replays the iteration from a hipGraph (helpers/step_helper.TrainIteration, the object bench.py times): three
        # eager iterations on real batches, the capture, then one launch per batch
        n_iter = 2 * len(trainer.train_loader)
        assert trainer.iteration.graph is not None and trainer.iteration.replays == n_iter - 3, (trainer.iteration.launch_mode(), trainer.iteration.replays)
        _check_train_val_outputs(tmp_path, ids)
        train_val.main(['--config', path, '-e'])                        # evaluation only, from checkpoint_epoch_2.pth
    finally:
        kernel_families.apply_switches(set())                           # module-level switches: leave the process as found


def _check_train_val_outputs(tmp_path, ids):
    out = tmp_path / 'outputs' / 'monodetr'
    # (checkpoint_best.pth is written only when the validation AP rises above 0, trainer_helper.py:100-107 -- not after two
    # epochs from random weights: the run keeps every epoch and the tester is pointed at the last one)
    assert (out / 'checkpoint_epoch_1.pth').exists() and (out / 'checkpoint_epoch_2.pth').exists()
    files = sorted(os.listdir(out / 'outputs' / 'data'))
    assert files == ['%s.txt' % i for i in ids]
    lines = [ln for f in files for ln in open(out / 'outputs' / 'data' / f).read().splitlines() if ln.strip()]
    assert lines                                                        # (a single image may have no detection after 12 iterations)
    line = lines[0].split(' ')
    assert len(line) == 16 and line[0] in ('Pedestrian', 'Car', 'Cyclist')


# ---- fused residual + dropout + LayerNorm ----------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C,dtype,p", [(81600, 256, torch.bfloat16, 0.1), (4400, 256, torch.float32, 0.0), (15360, 256, torch.float32, 0.1),
                                            (77, 128, torch.bfloat16, 0.0), (33, 512, torch.float32, 0.2)])
def test_fused_add_layernorm_kernel_matches_the_framework_operators(rows, C, dtype, p):
    from monodetr_amd import add_ln_ext
    from test_add_ln_emulated_cpu import keep_mask
    g = torch.Generator(device="cuda").manual_seed(rows + C)
    a = torch.randn(rows, C, generator=g, device="cuda").to(dtype).requires_grad_(True)
    b = (torch.randn(rows, C, generator=g, device="cuda") * 0.7 + 0.2).to(dtype).requires_grad_(True)
    gamma = (1 + 0.1 * torch.randn(C, generator=g, device="cuda")).requires_grad_(True)
    beta = (0.1 * torch.randn(C, generator=g, device="cuda")).requires_grad_(True)
    dy = torch.randn(rows, C, generator=g, device="cuda").to(dtype)
    y = add_ln_ext.fused_add_layernorm(a, b, gamma, beta, 1e-5, p, seed=987654321)
    y.backward(dy)
    got = (y.detach(), a.grad.clone(), b.grad.clone(), gamma.grad.clone(), beta.grad.clone())
    for t in (a, b, gamma, beta):
        t.grad = None
    keep = keep_mask(987654321, rows * C, p).view(rows, C).cuda() if p > 0 else torch.ones(rows, C, device="cuda")
    s = (a.float() + b.float() * keep / (1 - p)).to(dtype)
    ref = torch.nn.functional.layer_norm(s.float(), (C,), gamma, beta, 1e-5).to(dtype)
    ref.backward(dy)
    tol = 2e-2 if dtype == torch.bfloat16 else 2e-5
    for name, x, w in zip(("y", "da", "db", "dgamma", "dbeta"), got, (ref.detach(), a.grad, b.grad, gamma.grad, beta.grad)):
        scale = max(1.0, w.float().abs().max().item())
        lim = tol * scale * (30 if name in ("dgamma", "dbeta") and dtype == torch.bfloat16 else 1)      # sums of 81 600 bf16-rounded terms
        assert (x.float() - w.float()).abs().max().item() <= lim, name


def test_training_step_with_fused_layernorm_matches_default(monkeypatch):
    import bench
    from model_init import disable_dropout_
    from monodetr_amd import add_ln_ext
    dev = torch.device("cuda", 0)
    traj = {}
    for on in (False, True):
        monkeypatch.setattr(add_ln_ext, "ENABLED", on)
        step = bench.TrainStep(dev, 2, "bf16", size=(96, 320))
        disable_dropout_(step.raw_model)
        traj[on] = [float(step()) for _ in range(3)]
    for a, b in zip(traj[False], traj[True]):
        assert abs(a - b) <= 2e-2 * abs(a), traj


# ---- fused convolution / FFN tails (csrc/bias_act.hip) and ReLU in the library GEMM's epilogue ------------------------
@pytest.mark.parametrize("shape,dtype,bias_dtype,use_skip,p", [
    ((8, 64, 96, 320), torch.bfloat16, torch.bfloat16, False, 0.0),      # layer1 3x3 tail at the benchmark size
    ((8, 256, 96, 320), torch.bfloat16, None, True, 0.0),                # layer1 residual tail (126 MB per tensor)
    ((8, 2048, 12, 40), torch.float32, torch.float32, True, 0.0),
    ((3, 24, 7, 5), torch.float32, torch.float32, True, 0.0),            # 6 vectors per row: bias re-read per vector
    ((8, 10200, 256), torch.bfloat16, None, False, 0.1),                 # encoder FFN: ReLU + Dropout
    ((1920, 8, 256), torch.float32, None, False, 0.1),
])
def test_bias_act_kernel_matches_the_framework_operators(shape, dtype, bias_dtype, use_skip, p):
    from monodetr_amd import bias_act_ext
    from test_add_ln_emulated_cpu import keep_mask
    g = torch.Generator(device="cuda").manual_seed(sum(shape))
    cl = len(shape) == 4
    C = shape[1] if cl else shape[-1]

    def make():
        t = torch.randn(shape, generator=g, device="cuda").to(dtype)
        return t.contiguous(memory_format=torch.channels_last) if cl else t

    x, skip = make().requires_grad_(True), (make().requires_grad_(True) if use_skip else None)
    bias = (torch.randn(C, generator=g, device="cuda") * 0.5).to(bias_dtype) if bias_dtype is not None else None
    dy = make()
    y = bias_act_ext.bias_act(x, bias, skip, relu=True, dropout_p=p, seed=24680)
    assert y.stride() == x.stride()
    y.backward(dy)
    pre = x.detach().float() + (bias.float().view((1, C, 1, 1) if cl else (C,)) if bias is not None else 0.0) + (skip.detach().float() if use_skip else 0.0)
    if p > 0:
        keep = keep_mask(24680, x.numel(), p).view(shape).cuda()
        scale = torch.tensor(1.0 / (1.0 - p), dtype=torch.float32, device="cuda")
    else:
        keep, scale = torch.ones((), device="cuda"), torch.ones((), device="cuda")
    assert torch.equal(y.detach(), (torch.relu(pre) * scale * keep).to(dtype))
    want = torch.where((pre > 0) & (keep > 0), dy.float() * scale, torch.zeros((), device="cuda")).to(dtype)
    assert torch.equal(x.grad, want)
    if use_skip:
        assert torch.equal(skip.grad, want)


def test_library_gemm_relu_epilogue_matches_linear_then_relu_on_the_gpu(monkeypatch):
    from monodetr_amd.monodetr import linear
    torch.manual_seed(2)
    for dtype, T, K, N in ((torch.bfloat16, 81600, 256, 256), (torch.float32, 4400, 256, 256), (torch.bfloat16, 245760, 256, 64)):
        x = torch.randn(T, K, device="cuda").to(dtype).requires_grad_(True)
        w = (torch.randn(N, K, device="cuda") / 16).to(dtype).requires_grad_(True)
        b = torch.randn(N, device="cuda").to(dtype).requires_grad_(True)
        dy = torch.randn(T, N, device="cuda").to(dtype)
        monkeypatch.setattr(linear, "_GEMM_RELU", True)
        y = linear.token_linear(x, w, b, relu=True)
        assert y.grad_fn is not None and "TokenLinear" in type(y.grad_fn).__name__
        y.backward(dy)
        got = [y.detach(), x.grad.clone(), w.grad.clone(), b.grad.clone()]
        x.grad = w.grad = b.grad = None
        monkeypatch.setattr(linear, "_GEMM_RELU", False)
        ref = linear.token_linear(x, w, b, relu=True)
        ref.backward(dy)
        tol = 2e-2 if dtype == torch.bfloat16 else 1e-4
        for name, a, r in zip(("y", "dx", "dw", "db"), got, [ref.detach(), x.grad, w.grad, b.grad]):
            assert (a.float() - r.float()).abs().max().item() <= tol * max(1.0, r.float().abs().max().item()), (dtype, name)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_training_step_with_fused_tails_matches_default(monkeypatch, precision):
    import bench
    from model_init import disable_dropout_
    dev = torch.device("cuda", 0)
    traj = {}
    try:
        for names in ((), ("MDETR_FUSED_EPILOGUE",), ("MDETR_FUSED_EPILOGUE", "MDETR_GEMM_RELU")):
            step = bench.TrainStep(dev, 2, precision, size=(96, 320), switches=names)
            disable_dropout_(step.raw_model)
            traj[names] = [float(step()) for _ in range(3)]
    finally:
        bench.apply_switches(set())
    for names, t in traj.items():
        for a, b in zip(traj[()], t):
            assert abs(a - b) <= (2e-2 if precision == "bf16" else 2e-4) * abs(a), traj


# ---- implicit-GEMM 3x3 convolution (csrc/conv3x3.hip) ----------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C,N,relu", [(8, 96, 320, 64, 64, True), (8, 48, 160, 128, 128, True), (8, 24, 80, 256, 256, True),
                                             (8, 12, 40, 512, 512, False), (2, 13, 45, 64, 96, True)])
def test_conv3x3_kernel_matches_the_library_convolution(B, H, W, C, N, relu):
    from monodetr_amd import conv3x3_ext
    g = torch.Generator(device="cuda").manual_seed(C + N + H)
    x = torch.randn(B, C, H, W, generator=g, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    w = (torch.randn(N, C, 3, 3, generator=g, device="cuda") / (3.0 * C ** 0.5)).to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    shift = torch.randn(N, generator=g, device="cuda") * 0.5
    dy = torch.randn(B, N, H, W, generator=g, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    y = conv3x3_ext.conv3x3(x, w, shift, relu=relu)
    y.backward(dy)
    got = (y.detach(), x.grad.clone(), w.grad.clone())
    x.grad = w.grad = None
    from gemm_bounds import assert_product_close, conv2d_f64
    # fp64 on the same bf16 operands, ELEMENT-WISE: one bf16 rounding of the value + fp32 accumulation noise, the latter scaled by
    # the SAME operator applied to absolute values (round 4: 1.2e-2 / 4.8e-2 of the tensor's maximum)
    x64, w64 = x.detach().double().requires_grad_(True), w.detach().double().requires_grad_(True)
    pre = conv2d_f64(x64, w64, shift.double(), padding=1)
    ref = torch.relu(pre) if relu else pre
    mask = (y.detach() > 0) if relu else torch.ones_like(ref, dtype=torch.bool)
    gx, gw = torch.autograd.grad(pre, (x64, w64), dy.double() * mask)
    xa, wa = x.detach().double().abs().requires_grad_(True), w.detach().double().abs().requires_grad_(True)
    my = conv2d_f64(xa, wa, shift.double().abs(), padding=1)
    mx, mw = torch.autograd.grad(my, (xa, wa), dy.double().abs() * mask)
    for name, a, r, m, K in zip(("y", "dx", "dw"), got, (ref.detach(), gx, gw), (my.detach(), mx, mw), (9 * C, 9 * N, B * H * W)):
        if name == "dx" and N % 64 != 0:
            # (the input gradient's contraction runs over N: 96 channels are not whole slabs and go to the library, whose bf16 kernel
            # is not this repository's to hold to an ulp bound)
            assert ((a.double() - r).norm() / r.norm()).item() <= 1e-2
            continue
        assert_product_close(a, r, m, K, name)


def test_training_step_with_the_conv3x3_kernel_matches_default():
    import bench
    from model_init import disable_dropout_
    dev = torch.device("cuda", 0)
    traj = {}
    try:
        for names in ((), ("MDETR_CONV3X3",)):
            step = bench.TrainStep(dev, 2, "bf16", size=(96, 320), switches=names)
            disable_dropout_(step.raw_model)
            traj[names] = [float(step()) for _ in range(3)]
    finally:
        bench.apply_switches(set())
    for a, b in zip(traj[()], traj[("MDETR_CONV3X3",)]):
        assert abs(a - b) <= 2e-2 * abs(a), traj


def test_conv3x3_module_with_a_trainable_bias_matches_the_library(monkeypatch):
    """conv3x3_ext.Conv3x3 as the depth head uses it (bias with a gradient, no ReLU), kernel on vs off."""
    from monodetr_amd import conv3x3_ext
    torch.manual_seed(4)
    conv = conv3x3_ext.Conv3x3(256, 256, kernel_size=(3, 3), padding=1).cuda().to(torch.bfloat16).to(memory_format=torch.channels_last)
    x = torch.randn(8, 256, 24, 80, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    dy = torch.randn(8, 256, 24, 80, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    res = {}
    for on in (False, True):
        monkeypatch.setattr(conv3x3_ext, "ENABLED", on)
        xi = x.clone().requires_grad_(True)
        conv.zero_grad()
        y = conv(xi)
        assert (type(y.grad_fn).__name__ == "_Conv3x3Backward") == on
        y.backward(dy)
        res[on] = (y.detach(), xi.grad, conv.weight.grad.clone(), conv.bias.grad.clone())
    for name, a, b in zip(("y", "dx", "dw", "db"), res[False], res[True]):
        lim = 2e-2 * max(1.0, a.float().abs().max().item()) * (4 if name in ("dw", "db") else 1)       # bf16 sums over 15 360 pixels
        assert (a.float() - b.float()).abs().max().item() <= lim, name


# ---- strided convolutions (csrc/conv_taps.hip), convolution weight gradients (csrc/conv_wgrad.hip), the stem (csrc/conv_stem.hip) ----
@pytest.mark.parametrize("B,H,W,C,N,k,relu", [
    (8, 96, 320, 128, 128, 3, True),            # layer2.0.conv2
    (8, 48, 160, 256, 256, 3, True),            # layer3.0.conv2 (and the depth predictor's downsample)
    (8, 24, 80, 512, 512, 3, True),             # layer4.0.conv2
    (8, 12, 40, 2048, 256, 3, False),           # the fourth pyramid level (monodetr.py:87-92)
    (8, 96, 320, 256, 512, 1, False),           # layer2.0.downsample (1x1 / stride 2)
    (8, 24, 80, 1024, 2048, 1, False),          # layer4.0.downsample
    (2, 13, 45, 64, 192, 3, True),              # odd map, ragged tiles
    (8, 32, 110, 256, 256, 3, False),           # 512 x 1760: the depth predictor's downsample / level shapes of BASELINE configs[4]
])
def test_conv_strided_kernel_matches_the_library_convolution(B, H, W, C, N, k, relu, monkeypatch):
    from monodetr_amd import conv_taps_ext, conv_wgrad_ext
    monkeypatch.setattr(conv_wgrad_ext, "ENABLED", True)
    F = torch.nn.functional
    g = torch.Generator(device="cuda").manual_seed(C + N + H + k)
    pad = 1 if k == 3 else 0
    x = torch.randn(B, C, H, W, generator=g, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    w = (torch.randn(N, C, k, k, generator=g, device="cuda") / (k * C ** 0.5)).to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    shift = torch.randn(N, generator=g, device="cuda") * 0.5
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = torch.randn(B, N, OH, OW, generator=g, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    y = conv_taps_ext.conv_strided(x, w, shift, relu=relu)
    assert y.shape == (B, N, OH, OW)
    y.backward(dy)
    got = (y.detach(), x.grad.clone(), w.grad.clone())
    x.grad = w.grad = None
    from gemm_bounds import assert_product_close, conv2d_f64
    x64, w64 = x.detach().double().requires_grad_(True), w.detach().double().requires_grad_(True)
    pre = conv2d_f64(x64, w64, shift.double(), stride=2, padding=pad)                     # fp64 on the same bf16 operands
    ref = torch.relu(pre) if relu else pre
    mask = (y.detach() > 0) if relu else torch.ones_like(ref, dtype=torch.bool)
    gx, gw = torch.autograd.grad(pre, (x64, w64), dy.double() * mask)
    xa, wa = x.detach().double().abs().requires_grad_(True), w.detach().double().abs().requires_grad_(True)
    my = conv2d_f64(xa, wa, shift.double().abs(), stride=2, padding=pad)
    mx, mw = torch.autograd.grad(my, (xa, wa), dy.double().abs() * mask)
    for name, a, r, m, K in zip(("y", "dx", "dw"), got, (ref.detach(), gx, gw), (my.detach(), mx, mw), (k * k * C, k * k * N, B * OH * OW)):
        assert_product_close(a, r, m, K, name)                                            # element-wise (round 4: 1.2e-2 of the tensor's maximum)


@pytest.mark.parametrize("B,H,W,C,N", [(8, 48, 160, 128, 128), (8, 24, 80, 256, 256), (8, 12, 40, 512, 512), (2, 9, 37, 64, 96), (8, 32, 110, 256, 256)])
def test_conv_wgrad_kernel_matches_the_library_weight_gradient(B, H, W, C, N, monkeypatch):
    """csrc/conv_wgrad.hip at the stride-1 shapes of layer2-4 / the depth head: fp32 partial sums, ONE rounding -- held to the fp32
    autograd gradient on the same bf16 operands (tighter than the library's own bf16 split-K sums)."""
    from monodetr_amd import conv_wgrad_ext
    monkeypatch.setattr(conv_wgrad_ext, "ENABLED", True)
    g = torch.Generator(device="cuda").manual_seed(C + H)
    x = torch.randn(B, C, H, W, generator=g, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    dy = torch.randn(B, N, H, W, generator=g, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    assert conv_wgrad_ext.supported(x, dy, 3, 1)
    from gemm_bounds import assert_product_close, conv2d_f64
    w = torch.zeros(N, C, 3, 3, device="cuda", dtype=torch.float64, requires_grad=True)
    ref, = torch.autograd.grad(conv2d_f64(x.double(), w, None, padding=1), w, dy.double())
    mag, = torch.autograd.grad(conv2d_f64(x.double().abs(), w, None, padding=1), w, dy.double().abs())
    for dtype in (torch.float32, torch.bfloat16):
        dw = conv_wgrad_ext.weight_gradient(x, dy, 3, 1, dtype)
        assert dw.shape == ref.shape and dw.dtype == dtype
        assert_product_close(dw, ref, mag, B * H * W, str(dtype))                        # element-wise against fp64
    a, b = conv_wgrad_ext.weight_gradient(x, dy, 3, 1, torch.float32), conv_wgrad_ext.weight_gradient(x, dy, 3, 1, torch.float32)
    assert torch.equal(a, b)                                                             # fixed-order sums: deterministic


@pytest.mark.parametrize("form", ["1", "0"])
@pytest.mark.parametrize("T,K,N", [(81600, 256, 256), (81600, 256, 384), (61440, 128, 512), (15360, 1024, 256), (245760, 64, 256), (4408, 256, 256),
                                   (3840, 2048, 512), (245760, 256, 64), (4403, 264, 72)])
def test_token_wgrad_kernel_gives_weight_and_bias_gradient(T, K, N, form, monkeypatch):
    """mdetr_token_wgrad at the step's token shapes -- the encoder's 81 600 rows, the packed offsets / weights projection, the
    backbone's 1x1 convolutions -- as csrc/twgrad.hip (form 1: transposing LDS reads) and as the 1x1 case of csrc/conv_wgrad.hip
    (form 0), the bias gradient riding along: ELEMENT BY ELEMENT against the fp64 products of the same bf16 operands (fp32
    accumulation of exact products; bf16 results: one more rounding); deterministic."""
    from monodetr_amd import conv_wgrad_ext
    tune(monkeypatch, twgrad=form)
    monkeypatch.setattr(conv_wgrad_ext, "ENABLED", True)
    g = torch.Generator(device="cuda").manual_seed(T + N)
    x = (torch.randn(T, K, generator=g, device="cuda") * 0.5).to(torch.bfloat16)
    dy = (torch.randn(T, N, generator=g, device="cuda") * 0.1).to(torch.bfloat16)
    if not conv_wgrad_ext.token_supported(x, dy):
        pytest.skip("this form does not take the shape")
    rw, rb = dy.double().t() @ x.double(), dy.double().sum(0)
    mw, mb = dy.double().abs().t() @ x.double().abs(), dy.double().abs().sum(0)
    for dtype, ulp in ((torch.float32, 0.0), (torch.bfloat16, 2.0 ** -8)):
        dw, db = conv_wgrad_ext.token_weight_gradient(x, dy, dtype, bias=True)
        assert dw.shape == rw.shape and db.shape == rb.shape and dw.dtype == db.dtype == dtype
        assert bool(((dw.double() - rw).abs() <= ulp * rw.abs() + 4 * T ** 0.5 * 2.0 ** -23 * mw + 1e-30).all()), dtype
        assert bool(((db.double() - rb).abs() <= ulp * rb.abs() + 4 * T ** 0.5 * 2.0 ** -23 * mb + 1e-30).all()), dtype
    a, b = conv_wgrad_ext.token_weight_gradient(x, dy, torch.float32, bias=True), conv_wgrad_ext.token_weight_gradient(x, dy, torch.float32, bias=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("B,H,W", [(8, 384, 1280), (2, 512, 1760), (1, 37, 75)])
def test_conv_stem_kernel_matches_the_library_convolution(B, H, W):
    from monodetr_amd import conv_stem_ext
    g = torch.Generator(device="cuda").manual_seed(H)
    x = torch.randn(B, 3, H, W, generator=g, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(64, 3, 7, 7, generator=g, device="cuda") / 12).to(torch.bfloat16)
    shift = torch.randn(64, generator=g, device="cuda") * 0.3
    y = conv_stem_ext.conv_stem(x, w, shift)
    ref = torch.relu(torch.nn.functional.conv2d(x.float(), w.float(), shift, stride=2, padding=3))
    assert y.shape == ref.shape
    assert (y.float() - ref).abs().max().item() <= 1.2e-2 * max(1.0, ref.abs().max().item())
    # element by element against fp64 on the same bf16 operands: one bf16 rounding of an fp32-accumulated sum of 147 exact products
    from gemm_bounds import assert_product_close, conv2d_f64
    ref64 = torch.relu(conv2d_f64(x.double(), w.double(), shift.double(), stride=2, padding=3))
    mag64 = conv2d_f64(x.double().abs(), w.double().abs(), shift.double().abs(), stride=2, padding=3)
    assert_product_close(y, ref64, mag64, 147, "stem B=%d H=%d W=%d" % (B, H, W))


def _library_convolutions(step):
    """Which convolutions of one iteration still go to the library (shapes), for the failure message."""
    seen, F = [], torch.nn.functional
    real = F.conv2d

    def spy(x, w, *a, **k):
        seen.append((tuple(x.shape), tuple(w.shape), a[1:] if len(a) > 1 else k.get("stride")))
        return real(x, w, *a, **k)
    F.conv2d = spy
    try:
        step()
    finally:
        F.conv2d = real
    return seen


def test_training_step_with_the_convolution_kernels_matches_default():
    """The backbone / pyramid / depth-head convolutions by hand (stem, stride-2 3x3 and 1x1, every weight gradient) against the
    library path: loss trajectories of three iterations; and at the training resolution no MIOpen convolution is left in the
    iteration (at 96 x 320 the depth predictor's 6 x 20 maps fall below what the GroupNorm kernel takes, the framework's GroupNorm
    hands NCHW-contiguous maps on, and the convolutions behind it rightly stay with the library)."""
    import bench
    from model_init import disable_dropout_
    dev = torch.device("cuda", 0)
    traj, families = {}, ("MDETR_CONV3X3", "MDETR_CONV_STRIDED", "MDETR_CONV_WGRAD", "MDETR_CONV_STEM")
    try:
        for names in ((), families):
            step = bench.TrainStep(dev, 2, "bf16", size=(96, 320), switches=names)
            disable_dropout_(step.raw_model)
            traj[names] = [float(step()) for _ in range(3)]
            del step
        step = bench.TrainStep(dev, 1, "bf16", size=(384, 1280), switches=set(bench.COMMITTED_SWITCHES["bf16"]) | set(families))
        step()
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        kernels = [e.key for e in prof.key_averages()]
        left = [k for k in kernels if "igemm" in k or "miopen" in k.lower() or "conv_bwd" in k or "grouped_conv" in k or "SubTensorOp" in k]
        seen = _library_convolutions(step) if left else []
        if left:
            os.makedirs("gpurun_out", exist_ok=True)
            with open("gpurun_out/library_convolutions.txt", "w") as f:
                f.write("\n".join(map(str, left)) + "\n" + "\n".join(map(str, seen)) + "\n")
        assert not left, (left, seen[:12])
        assert any("conv_wgrad_kernel" in k for k in kernels) and any("conv_taps_kernel" in k for k in kernels) and any("conv_stem_kernel" in k for k in kernels)
        assert any("conv_dgrad4_kernel" in k for k in kernels)
    finally:
        bench.apply_switches(set())
    for a, b in zip(traj[()], traj[families]):
        assert abs(a - b) <= 2e-2 * abs(a), traj


# ---- GroupNorm (+ ReLU) on channels-last activations (csrc/group_norm.hip) --------------------------------------------------
@pytest.mark.parametrize("shape,dtype,pdtype,relu", [
    ((8, 256, 24, 80), torch.bfloat16, torch.bfloat16, True),          # depth head stage
    ((8, 256, 48, 160), torch.bfloat16, torch.bfloat16, False),        # input projection, level 0: 32 row chunks of 240
    ((8, 256, 6, 20), torch.bfloat16, torch.float32, False),           # coarsest level
    ((2, 256, 24, 80), torch.float32, torch.float32, True),            # the fp32 path
])
def test_group_norm_kernel_matches_the_framework_operator(shape, dtype, pdtype, relu):
    import torch.nn.functional as F
    from monodetr_amd import group_norm_ext
    g = torch.Generator(device="cuda").manual_seed(sum(shape))
    N, C, H, W = shape
    x = (torch.randn(shape, device="cuda", generator=g) * 1.7 + 0.3).to(dtype).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    w = (torch.randn(C, device="cuda", generator=g) * 0.5 + 1.0).to(pdtype).requires_grad_(True)
    b = (torch.randn(C, device="cuda", generator=g) * 0.5).to(pdtype).requires_grad_(True)
    dy = torch.randn(shape, device="cuda", generator=g).to(dtype).contiguous(memory_format=torch.channels_last)
    y = group_norm_ext.group_norm(x, w, b, 32, 1e-5, relu)
    assert type(y.grad_fn).__name__ == "_GroupNormBackward" and y.is_contiguous(memory_format=torch.channels_last) and y.dtype == dtype
    y.backward(dy)
    got = (y.detach().float(), x.grad.float(), w.grad.float(), b.grad.float())
    xr, wr, br = (t.detach().float().requires_grad_(True) for t in (x, w, b))
    ref = F.group_norm(xr, 32, wr, br, 1e-5)
    pre = ref.detach()
    if relu:
        ref = F.relu(ref)
    ref.backward(dy.float())
    out_tol = 2 ** -8 if dtype == torch.bfloat16 else 2e-5
    for name, a, r in zip(("y", "dx", "dw", "db"), got, (ref.detach(), xr.grad, wr.grad, br.grad)):
        tol = out_tol * (8 if name in ("dw", "db") else 1)            # sums over N * HW pixels, rounded once (bf16 parameters)
        if relu and name == "dx":
            near = pre.abs() < 1e-3                                    # elements whose mask may round the other way
            a, r = a.masked_fill(near, 0.0), r.masked_fill(near, 0.0)
            tol *= 4
        assert (a - r).abs().max().item() <= tol * max(1.0, r.abs().max().item()), name


def test_training_step_with_the_group_norm_kernel_matches_default():
    import bench
    from model_init import disable_dropout_
    dev = torch.device("cuda", 0)
    traj = {}
    try:
        for names in ((), ("MDETR_GROUP_NORM",)):
            step = bench.TrainStep(dev, 2, "bf16", size=(96, 320), switches=names)
            disable_dropout_(step.raw_model)
            traj[names] = [float(step()) for _ in range(3)]
    finally:
        bench.apply_switches(set())
    for a, b in zip(traj[()], traj[("MDETR_GROUP_NORM",)]):
        assert abs(a - b) <= 2e-2 * abs(a), traj


# ---- weight / bias gradient over a few thousand token rows (csrc/small_wgrad.hip) -------------------------------------------
@pytest.mark.parametrize("T,N,K,dtype", [(4400, 256, 256, torch.bfloat16), (4400, 512, 256, torch.bfloat16), (4400, 128, 256, torch.bfloat16),
                                         (4400, 256, 256, torch.float32), (8192, 256, 256, torch.bfloat16), (130, 64, 64, torch.bfloat16)])
def test_small_wgrad_kernel_matches_the_library_products(T, N, K, dtype):
    from monodetr_amd import small_wgrad_ext
    g = torch.Generator(device="cuda").manual_seed(T + N + K)
    dy, x = torch.randn(T, N, device="cuda", generator=g).to(dtype), torch.randn(T, K, device="cuda", generator=g).to(dtype)
    dw, db = small_wgrad_ext.small_wgrad(dy, x, dtype)
    rw, rb = dy.double().t() @ x.double(), dy.double().sum(0)
    tol = 2 ** -8 if dtype == torch.bfloat16 else 1e-5
    assert (dw.double() - rw).abs().max() <= tol * rw.abs().max() and (db.double() - rb).abs().max() <= tol * max(1.0, rb.abs().max().item())
    from gemm_bounds import assert_product_close
    assert_product_close(dw, rw, dy.double().abs().t() @ x.double().abs(), T, "small_wgrad dW")       # element-wise: fp32 sums over T rows, one rounding
    assert_product_close(db, rb, dy.double().abs().sum(0), T, "small_wgrad db")
    dw2, db2 = small_wgrad_ext.small_wgrad(dy, x, dtype)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)                    # fixed summation order: deterministic


def test_training_step_with_the_small_wgrad_kernel_matches_default():
    import bench
    from model_init import disable_dropout_
    dev = torch.device("cuda", 0)
    traj = {}
    try:
        for names in ((), ("MDETR_SMALL_WGRAD",)):
            step = bench.TrainStep(dev, 8, "bf16", size=(96, 320), switches=names)      # B = 8: 4 400 decoder rows, the kernel's case
            disable_dropout_(step.raw_model)
            traj[names] = [float(step()) for _ in range(3)]
    finally:
        bench.apply_switches(set())
    for a, b in zip(traj[()], traj[("MDETR_SMALL_WGRAD",)]):
        assert abs(a - b) <= 2e-2 * abs(a), traj


@pytest.mark.parametrize("B,C,H,W,dtype", [(8, 256, 96, 320, torch.bfloat16), (2, 1024, 24, 80, torch.bfloat16), (1, 8, 7, 9, torch.float32)])
def test_decimate_kernel_and_the_projection_shortcut_as_a_token_gemm(B, C, H, W, dtype):
    """csrc/decimate.hip on the GPU: x[:, :, ::2, ::2] and its adjoint bit-exact against slicing; conv_bn's 1x1 / stride-2
    route (gather + token GEMM) against the library convolution on the same bf16 operands."""
    from monodetr_amd import decimate_ext
    g = torch.Generator(device="cuda").manual_seed(C + H)
    x = torch.randn(B, C, H, W, device="cuda", generator=g).to(dtype).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = decimate_ext.decimate2(x)
    assert torch.equal(y, x.detach()[:, :, ::2, ::2])
    gy = torch.randn(y.shape, device="cuda", generator=g).to(dtype)
    (gx,) = torch.autograd.grad(y, x, gy)
    ref = torch.zeros_like(x.detach())
    ref[:, :, ::2, ::2] = gy
    assert torch.equal(gx, ref)
    if dtype == torch.bfloat16:
        N = 2 * C
        w = (torch.randn(N, C, 1, 1, device="cuda", generator=g) / C ** 0.5).to(dtype).requires_grad_(True)
        b = torch.randn(N, device="cuda", generator=g).to(dtype)
        from monodetr_amd.monodetr.linear import pointwise_conv
        got = pointwise_conv(decimate_ext.decimate2(x), w, b)
        want = torch.nn.functional.conv2d(x.float(), w.float(), b.float(), stride=2)
        assert (got.float() - want).abs().max() <= 2e-2 * want.abs().max()
        go = torch.randn(got.shape, device="cuda", generator=g).to(dtype)
        grads = torch.autograd.grad(got, [x, w], go)
        for a, c in zip(grads, torch.autograd.grad(want, [x, w], go.float())):
            assert (a.float() - c.float()).abs().max() <= 2e-2 * c.float().abs().max()
        # element by element against fp64 on the same bf16 operands (one rounding of an fp32-accumulated product each)
        from gemm_bounds import assert_product_close, conv2d_f64
        from monodetr_amd import small_wgrad_ext
        x64, w64 = x.detach().double().requires_grad_(True), w.detach().double().requires_grad_(True)
        ref = conv2d_f64(x64, w64, b.double(), stride=2)
        gx, gw = torch.autograd.grad(ref, (x64, w64), go.double())
        xa, wa = x.detach().double().abs().requires_grad_(True), w.detach().double().abs().requires_grad_(True)
        mag = conv2d_f64(xa, wa, b.double().abs(), stride=2)
        mx, mw = torch.autograd.grad(mag, (xa, wa), go.double().abs())
        T = got.numel() // N
        assert_product_close(got, ref.detach(), mag.detach(), C, "decimate route y")
        assert_product_close(grads[0], gx, mx, N, "decimate route dx")
        if T <= small_wgrad_ext.MAX_ROWS:       # (beyond it the library route rounds each of its split-K chunk products to bf16: not ONE rounding)
            assert_product_close(grads[1], gw, mw, T, "decimate route dw")


@pytest.mark.parametrize("B,C,H,W", [(8, 64, 192, 640), (1, 8, 7, 9), (2, 64, 5, 6)])
def test_maxpool_kernel_matches_the_framework(B, C, H, W):
    """csrc/decimate.hip maxpool3x3s2_bf16 (the frozen stem's pooling) == F.max_pool2d(x, 3, 2, 1), bit for bit."""
    from monodetr_amd import decimate_ext
    g = torch.Generator(device="cuda").manual_seed(H + W)
    x = torch.randn(B, C, H, W, device="cuda", generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    assert decimate_ext.maxpool_supported(x)
    y = decimate_ext.maxpool3x3s2(x)
    want = torch.nn.functional.max_pool2d(x, 3, 2, 1)
    assert y.shape == want.shape and torch.equal(y, want)


# ---- the frozen-BN fold of the trainable backbone weights in one launch each way (csrc/wfold.hip) ------------------------------------
def test_fold_kernel_matches_the_multi_tensor_fold():
    """Every trainable convolution of a ResNet-50 body at once: folded weights, [C][tap][O] copies and unfolded gradients, bit for
    bit the framework expressions they replace."""
    from monodetr_amd import wfold_ext
    g = torch.Generator(device="cuda").manual_seed(5)
    shapes = []
    for planes, blocks in ((128, 4), (256, 6), (512, 3)):
        for b in range(blocks):
            cin = planes * 2 if b == 0 else planes * 4
            shapes += [(planes, cin, 1, 1), (planes, planes, 3, 3), (planes * 4, planes, 1, 1)]
        shapes.append((planes * 4, planes * 2, 1, 1))
    ws = [(torch.randn(*s, device="cuda", generator=g) * 0.05).contiguous(memory_format=torch.channels_last) for s in shapes]
    ss = [torch.rand(s[0], device="cuda", generator=g) + 0.5 for s in shapes]
    want_t = [s[2] == 3 for s in shapes]
    assert len(ws) == 42 and wfold_ext.supported(ws, ss, torch.bfloat16)
    folded, folded_t = wfold_ext.fold_weights(ws, ss, want_t)
    for w, s, f, ft in zip(ws, ss, folded, folded_t):
        ref = (w * s.view(-1, 1, 1, 1)).to(torch.bfloat16)
        assert torch.equal(f, ref) and f.shape == w.shape
        assert (ft is None) == (w.shape[2] == 1)
        if ft is not None:
            assert ft.is_contiguous() and torch.equal(ft, ref.permute(1, 2, 3, 0))
    grads = [torch.randn(*s, device="cuda", generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last) for s in shapes]
    assert wfold_ext.grads_supported(grads, ws)
    for w, s, gr, o in zip(ws, ss, grads, wfold_ext.unfold_grads(grads, ss, ws)):
        assert o.dtype == torch.float32 and torch.equal(o, gr.float() * s.view(-1, 1, 1, 1))


def test_training_step_with_the_fold_kernel_matches_default():
    """The committed bf16 list with and without MDETR_WFOLD: the same folded weights and the same unfolded gradients, so the
    loss trajectories coincide to the last bit that deterministic kernels leave (dropout off)."""
    import bench
    from model_init import disable_dropout_
    dev = torch.device("cuda", 0)
    base = tuple(sorted(set(bench.COMMITTED_SWITCHES["bf16"]) - {"MDETR_WFOLD"}))
    traj = {}
    try:
        for names in (base, base + ("MDETR_WFOLD",)):
            step = bench.TrainStep(dev, 2, "bf16", size=(96, 320), switches=names)
            disable_dropout_(step.raw_model)
            traj[names] = [float(step()) for _ in range(3)]
    finally:
        bench.apply_switches(set())
    for a, b in zip(traj[base], traj[base + ("MDETR_WFOLD",)]):
        assert abs(a - b) <= 1e-3 * abs(a), traj
