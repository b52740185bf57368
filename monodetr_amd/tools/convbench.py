"""Op-level timing of the hand-written convolutions (csrc/conv3x3.hip, conv_taps.hip, conv_wgrad.hip, conv_stem.hip) against the
library convolutions they replace (MIOpen through aten), at the shapes of the training step: B = 8, 3 x 384 x 1280, bf16
channels_last.  TFLOP/s = 2 B OH OW K K C N / t; `frac_mfma` against the 2.5 PFLOP/s dense bf16 rate.

    python -m monodetr_amd.tools.convbench [--iters 20] [--only wgrad|strided|stem]
    python -m monodetr_amd.tools.convbench --dtype fp32 [--runs 3]      (the fp32 forms of conv3x3.hip / conv_wgrad.hip against the library: `fp32_rows`;
                                                                         the weight-gradient rows include the 3x3 / stride-2 sites, `..._s2`)
    python -m monodetr_amd.tools.convbench --dtype fp32 --only strided  (the fp32 form of conv_taps.hip on the model's stride-2 3x3 sites: `fp32_strided_rows`)
    python -m monodetr_amd.tools.convbench --dtype fp32 --only stem     (the fp32 form of conv_stem.hip against the library convolution + the shift / ReLU pass: `fp32_stem_rows`)
"""
import argparse
import json

import torch
import torch.nn.functional as F

from .fusedbench import timeit


def rec(ms, flops):
    return dict(ms=round(ms, 4), TFLOPs=round(flops / ms / 1e9, 1), frac_mfma=round(flops / (ms * 1e-3) / 2.5e15, 4))


def fp32_rows(a, dev, B):
    """--dtype fp32: the fp32 forms of csrc/conv3x3.hip (mdetr_conv3x3_f32) and csrc/conv_wgrad.hip (mdetr_conv_wgrad_f32 + its chunk sum)
    against the library route of an fp32 stride-1 3x3 convolution -- forward with the library's bias and ReLU passes, the input
    gradient and the weight gradient -- in one process, as graph replays over two operand
    sets: per row the median of --runs captures (best replay of each) with the spread, and the fraction of the six-term matrix-instruction
    bound 6 x flops / 2.5 PFLOP/s the kernel reaches."""
    import statistics
    from monodetr_amd import conv3x3_ext, conv_wgrad_ext
    from .gemmbench import graph_time
    conv3x3_ext.ENABLED_F32 = True
    conv_wgrad_ext.ENABLED_CONV_F32 = True
    shapes = (("layer1", 64, 96, 320), ("layer2", 128, 48, 160), ("layer3", 256, 24, 80), ("layer4", 512, 12, 40), ("depth_head", 256, 24, 80))
    res, nsets, reps = {}, 2, max(4, a.iters)

    def row(f, flops):
        us = sorted(graph_time(f, nsets, reps) for _ in range(a.runs))
        med = statistics.median(us)
        return dict(us=round(med, 2), spread_us=[us[0], us[-1]], TFLOPs=round(flops / med / 1e6, 1), frac_six_term_mfma=round(6.0 * flops / (med * 1e-6) / 2.5e15, 4))

    done = set()
    for tag, C, H, W in shapes:
        if (C, H, W) in done:                                           # (the depth head's 256 -> 256 at 24 x 80 is layer3's problem)
            res["f32_%s" % tag] = "same problem as layer3"
            continue
        done.add((C, H, W))
        flops = 2.0 * B * H * W * 9 * C * C
        xs = [(torch.randn(B, H, W, C, device=dev) * 0.5).permute(0, 3, 1, 2) for _ in range(nsets)]
        dys = [torch.randn(B, H, W, C, device=dev).permute(0, 3, 1, 2) for _ in range(nsets)]
        w = (torch.randn(C, 3, 3, C, device=dev) / (3.0 * C ** 0.5)).permute(0, 3, 1, 2)
        sh = torch.randn(C, device=dev) * 0.5
        assert conv3x3_ext.supported_f32(xs[0], w)
        wo, wt = conv3x3_ext._ohwi(w), conv3x3_ext._ohwi(w).permute(3, 1, 2, 0).contiguous()
        if a.only != "wgrad":                                          # (--only wgrad: the weight-gradient rows alone)
            res["f32_fwd_%s_kernel" % tag] = row(lambda i: conv3x3_ext._launch(xs[i], wo, sh, True), flops)
            res["f32_fwd_%s_library" % tag] = row(lambda i: F.relu_(F.conv2d(xs[i], w, sh, padding=1)), flops)
            res["f32_dgrad_%s_kernel" % tag] = row(lambda i: conv3x3_ext._launch(dys[i], wt, None, False, mirror=True), flops)
            res["f32_dgrad_%s_library" % tag] = row(lambda i: torch.ops.aten.convolution_backward(
                dys[i], xs[i], w, None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1, (True, False, False)), flops)
            res["f32_%s_plan" % tag] = conv3x3_ext._lib().mdetr_conv3x3_f32_plan(B, H, W, C)
        # the weight gradient: the fp32 form of csrc/conv_wgrad.hip (mdetr_conv_wgrad_f32) + the sum over its chunks against the library's
        res["f32_wgrad_%s_routed_to_kernel" % tag] = bool(conv_wgrad_ext.supported_f32(xs[0], dys[0], 3, 1))     # (the shape rule; both are timed)
        res["f32_wgrad_%s_kernel" % tag] = row(lambda i: conv_wgrad_ext.weight_gradient(xs[i], dys[i], 3, 1, torch.float32), flops)
        res["f32_wgrad_%s_library" % tag] = row(lambda i: torch.ops.aten.convolution_backward(
            dys[i], xs[i], w, None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1, (False, True, False)), flops)
        res["f32_wgrad_%s_chunks" % tag] = conv_wgrad_ext._lib().mdetr_conv_wgrad_f32_chunks(B, H, W, C, H, W, C, 3, 1)
    # the 3x3 / stride-2 sites (layer2.0 / layer3.0 / layer4.0 conv2; the depth predictor's downsample is layer3.0's problem): the
    # stride-2 form (mdetr_conv_wgrad_s2_f32) + the sum over its chunks against the library's weight gradient at stride 2, (H, W) the INPUT
    conv_wgrad_ext.ENABLED_CONV_S2_F32 = True
    for tag, C, H, W in (("layer2_s2", 128, 96, 320), ("layer3_s2", 256, 48, 160), ("layer4_s2", 512, 24, 80)):
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        flops = 2.0 * B * OH * OW * 9 * C * C
        xs = [(torch.randn(B, H, W, C, device=dev) * 0.5).permute(0, 3, 1, 2) for _ in range(nsets)]
        dys = [torch.randn(B, OH, OW, C, device=dev).permute(0, 3, 1, 2) for _ in range(nsets)]
        w = (torch.randn(C, 3, 3, C, device=dev) / (3.0 * C ** 0.5)).permute(0, 3, 1, 2)
        res["f32_wgrad_%s_routed_to_kernel" % tag] = bool(conv_wgrad_ext.supported_f32_s2(xs[0], dys[0]))       # (the shape rule; both are timed)
        res["f32_wgrad_%s_kernel" % tag] = row(lambda i: conv_wgrad_ext.weight_gradient(xs[i], dys[i], 3, 2, torch.float32), flops)
        res["f32_wgrad_%s_library" % tag] = row(lambda i: torch.ops.aten.convolution_backward(
            dys[i], xs[i], w, None, (2, 2), (1, 1), (1, 1), False, (0, 0), 1, (False, True, False)), flops)
        res["f32_wgrad_%s_chunks" % tag] = conv_wgrad_ext._lib().mdetr_conv_wgrad_s2_f32_chunks(B, H, W, C, OH, OW, C, 3, 2)
    return res


def strided_sites(dev, B, size=(384, 1280)):
    """(name, C, N, H, W) of every 3x3 / stride-2 / pad-1 convolution of the model, read from the modules during one fp32 training
    iteration at batch B: a Bottleneck whose conv2 strides sees conv2's input size at its own input (conv1 is 1x1 / stride 1); the
    pyramid level and the depth predictor's downsample are modules of their own."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
    import bench
    from monodetr_amd.kernel_families import COMMITTED_SWITCHES
    from monodetr_amd.monodetr.backbone import Bottleneck
    step = bench.TrainStep(torch.device(dev), B, "fp32", switches=COMMITTED_SWITCHES["fp32"], graph=False, size=size)
    is_site = lambda m: isinstance(m, torch.nn.Conv2d) and tuple(m.kernel_size) == (3, 3) and tuple(m.stride) == (2, 2) \
        and tuple(m.padding) == (1, 1) and m.groups == 1                # noqa: E731
    sites, hooks, inside = [], [], set()

    def note(name, conv):
        def hook(mod, args):
            sites.append((name, conv.in_channels, conv.out_channels, int(args[0].shape[2]), int(args[0].shape[3])))
        return hook
    for name, m in step.raw_model.named_modules():
        if isinstance(m, Bottleneck) and is_site(m.conv2):
            hooks.append(m.register_forward_pre_hook(note(name + ".conv2", m.conv2)))
            inside.add(m.conv2)
    for name, m in step.raw_model.named_modules():
        if is_site(m) and m not in inside:
            hooks.append(m.register_forward_pre_hook(note(name, m)))
    step()
    for h in hooks:
        h.remove()
    del step
    return sites


def fp32_strided_rows(a, dev, B):
    """--dtype fp32 --only strided: the fp32 form of csrc/conv_taps.hip (mdetr_conv_taps_f32 / its split form + the sum over the splits,
    mdetr_conv_dgrad_s2_f32) against the library route -- F.conv2d(stride=2) + bias + ReLU forward, convolution_backward(..., (True,
    False, False)) for dX -- on every 3x3 / stride-2 site of the model (`strided_sites`), by the method of `fp32_rows`.  The pyramid
    level (no ReLU: GroupNorm follows) is timed with and without the contraction split.  Every class is timed whatever the shape rule of
    conv_taps_ext says; what the rule routes is reported beside it (`..._routed_to_kernel`)."""
    import statistics
    from monodetr_amd import _tune, conv_taps_ext
    from .gemmbench import graph_time
    sites = strided_sites(dev, B)
    conv_taps_ext.ENABLED_F32 = True
    res, nsets, reps = {"sites": [list(s) for s in sites], "tune": _tune.get("conv_taps_f32_rows", "") + "/" + _tune.get("conv_taps_f32_nb", "")}, 2, max(4, a.iters)

    def row(f, flops):
        us = sorted(graph_time(f, nsets, reps) for _ in range(a.runs))
        med = statistics.median(us)
        return dict(us=round(med, 2), spread_us=[us[0], us[-1]], TFLOPs=round(flops / med / 1e6, 1), frac_six_term_mfma=round(6.0 * flops / (med * 1e-6) / 2.5e15, 4))

    done = {}
    for name, C, N, H, W in sites:
        if (C, N, H, W) in done:
            res["f32_%s" % name] = "same problem as " + done[(C, N, H, W)]
            continue
        done[(C, N, H, W)] = name
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        flops = 2.0 * B * OH * OW * 9 * C * N
        xs = [(torch.randn(B, H, W, C, device=dev) * 0.5).permute(0, 3, 1, 2) for _ in range(nsets)]
        dys = [torch.randn(B, OH, OW, N, device=dev).permute(0, 3, 1, 2) for _ in range(nsets)]
        w = (torch.randn(N, 3, 3, C, device=dev) / (3.0 * C ** 0.5)).permute(0, 3, 1, 2)
        sh = torch.randn(N, device=dev) * 0.5
        # the measured shape rule (conv_taps_ext._F32_FWD_MAX_C / _F32_DX_MAX_C) is reported per class; both classes are timed all the same
        res["f32_%s_routed_to_kernel" % name] = dict(supported=bool(conv_taps_ext.supported_f32(xs[0], w)), forward=bool(conv_taps_ext._fwd_on_kernel(xs[0])),
                                                      dgrad=bool(conv_taps_ext._dx_on_kernel(dys[0], C)))
        rule = (conv_taps_ext._F32_FWD_MAX_C, conv_taps_ext._F32_DX_MAX_C)
        conv_taps_ext._F32_FWD_MAX_C = conv_taps_ext._F32_DX_MAX_C = 1 << 30
        assert conv_taps_ext.supported_f32(xs[0], w), name                 # (dtype, layout and the entry's limits)
        conv_taps_ext._F32_FWD_MAX_C, conv_taps_ext._F32_DX_MAX_C = rule
        wo = conv_taps_ext._ohwi(w)                                        # (a view: the weight is channels_last, as the model's are on the GPU)
        wt = wo.permute(3, 1, 2, 0).contiguous()
        relu = not name.startswith("input_proj")
        ks = conv_taps_ext._split_count(B, OH, OW, N, C, 3, relu)
        res["f32_fwd_%s_kernel" % name] = dict(row(lambda i: conv_taps_ext._forward(xs[i], wo, sh, relu), flops), ksplit=ks)
        if ks:
            with _no_split():
                res["f32_fwd_%s_kernel_unsplit" % name] = row(lambda i: conv_taps_ext._forward(xs[i], wo, sh, relu), flops)
        lib_fwd = (lambda i: F.relu_(F.conv2d(xs[i], w, sh, stride=2, padding=1))) if relu else (lambda i: F.conv2d(xs[i], w, sh, stride=2, padding=1))
        res["f32_fwd_%s_library" % name] = row(lib_fwd, flops)
        res["f32_dgrad_%s_kernel" % name] = row(lambda i: conv_taps_ext._input_gradient(dys[i], wo, H, W, wt), flops)
        # as the routed autograd node runs it: fp32 weights carry no [C, 3, 3, N] copy (`_mdetr_ihwo` is made by the bf16 fold kernel only),
        # so every backward pass transposes the weight first
        res["f32_dgrad_%s_kernel_with_weight_transpose" % name] = row(lambda i: conv_taps_ext._input_gradient(dys[i], wo, H, W), flops)
        res["f32_dgrad_%s_library" % name] = row(lambda i: torch.ops.aten.convolution_backward(
            dys[i], xs[i], w, None, (2, 2), (1, 1), (1, 1), False, (0, 0), 1, (True, False, False)), flops)
    return res


def fp32_stem_rows(a, dev, B, sizes=((384, 1280), (512, 1760))):
    """--dtype fp32 --only stem: the fp32 form of csrc/conv_stem.hip (mdetr_conv_stem_f32: convolution, shift and ReLU in one launch) against
    the library route of backbone.conv_bn on the same fp32 operands -- F.conv2d, then bias_act_ext.bias_act(..., relu=True) --, at the image
    sizes of the two fp32 configurations, by the method of `fp32_rows`."""
    import statistics
    from monodetr_amd import bias_act_ext, conv_stem_ext
    from .gemmbench import graph_time
    conv_stem_ext.ENABLED_F32 = True
    res, nsets, reps = {}, 2, max(4, a.iters)

    def row(f, flops):
        us = sorted(graph_time(f, nsets, reps) for _ in range(a.runs))
        med = statistics.median(us)
        return dict(us=round(med, 2), spread_us=[us[0], us[-1]], TFLOPs=round(flops / med / 1e6, 1), frac_six_term_mfma=round(6.0 * flops / (med * 1e-6) / 2.5e15, 4))

    for H, W in sizes:
        tag = "%dx%d" % (H, W)
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        flops = 2.0 * B * OH * OW * 64 * 147
        xs = [torch.randn(B, H, W, 3, device=dev).permute(0, 3, 1, 2) for _ in range(nsets)]
        w = (torch.randn(64, 7, 7, 3, device=dev) / 12.0).permute(0, 3, 1, 2)
        sh = torch.randn(64, device=dev) * 0.3
        assert conv_stem_ext.supported_f32(xs[0], w)
        planes = conv_stem_ext.pack_weight_f32(w)
        y = F.conv2d(xs[0], w, None, stride=2, padding=3)
        assert bias_act_ext.supported(y, sh)                               # (the pass conv_bn runs behind the library convolution in fp32)
        res["f32_stem_%s_kernel" % tag] = row(lambda i: conv_stem_ext._launch_f32(xs[i], planes, sh, True), flops)
        res["f32_stem_%s_library" % tag] = row(lambda i: bias_act_ext.bias_act(F.conv2d(xs[i], w, None, stride=2, padding=3), sh, None, relu=True), flops)
        res["f32_stem_%s_library_conv_alone" % tag] = row(lambda i: F.conv2d(xs[i], w, None, stride=2, padding=3), flops)
        k, lib = res["f32_stem_%s_kernel" % tag], res["f32_stem_%s_library" % tag]
        res["f32_stem_%s_kernel_ahead" % tag] = bool(k["us"] < lib["spread_us"][0])      # the median ahead of the library route's own [min, max]
    return res


class _no_split:
    """MDETR_TUNE conv_taps_split=0 for the duration of a block (the unsplit forward of a site the route would split)."""

    def __enter__(self):
        import os
        self.old = os.environ.get("MDETR_TUNE")
        os.environ["MDETR_TUNE"] = ",".join(x for x in (self.old, "conv_taps_split=0") if x)

    def __exit__(self, *exc):
        import os
        if self.old is None:
            os.environ.pop("MDETR_TUNE", None)
        else:
            os.environ["MDETR_TUNE"] = self.old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--only", default="")
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp32"))
    ap.add_argument("--runs", type=int, default=3, help="--dtype fp32: graph captures per row (median and spread are reported)")
    a = ap.parse_args()
    dev, B = "cuda", a.batch
    from monodetr_amd import conv3x3_ext, conv_taps_ext, conv_wgrad_ext
    if a.dtype == "fp32":
        print(json.dumps(fp32_strided_rows(a, dev, B) if a.only == "strided" else fp32_stem_rows(a, dev, B) if a.only == "stem" else fp32_rows(a, dev, B)))
        return
    conv_wgrad_ext.ENABLED = True
    res = {}

    def tensors(C, N, H, W, k, stride):
        pad = 1 if k == 3 else 0
        OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        x = torch.randn(B, C, H, W, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        w = (torch.randn(N, C, k, k, device=dev) / (k * C ** 0.5)).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        dy = torch.randn(B, N, OH, OW, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        return x, w, dy, pad, 2.0 * B * OH * OW * k * k * C * N

    # ---- forward / input gradient, 3x3 stride 1 (csrc/conv3x3.hip), kernel only: the PMC passes of scripts/r03_*.sh profile this ----
    if a.only == "conv3x3":
        for tag, (C, H, W) in (("layer1", (64, 96, 320)), ("layer2", (128, 48, 160)), ("layer3", (256, 24, 80)), ("layer4", (512, 12, 40))):
            x, w, dy, pad, flops = tensors(C, C, H, W, 3, 1)
            sh = torch.randn(C, device=dev)
            wo = conv3x3_ext._ohwi(w)
            res["conv3x3_%s_kernel" % tag] = rec(timeit(lambda: conv3x3_ext._launch(x, wo, sh, True), a.iters), flops)
            res["wgrad3x3_%s_kernel" % tag] = rec(timeit(lambda: conv_wgrad_ext.weight_gradient(x, dy, 3, 1, torch.bfloat16), a.iters), flops)

    # ---- weight gradient, 3x3 stride 1: the 10 trainable Bottleneck.conv2 of layer2-4 and the depth head's two convolutions ----
    if a.only in ("", "wgrad"):
        for tag, (C, H, W) in (("layer2", (128, 48, 160)), ("layer3", (256, 24, 80)), ("layer4", (512, 12, 40))):
            x, w, dy, pad, flops = tensors(C, C, H, W, 3, 1)
            res["wgrad3x3_%s_kernel" % tag] = rec(timeit(lambda: conv_wgrad_ext.weight_gradient(x, dy, 3, 1, torch.bfloat16), a.iters), flops)
            res["wgrad3x3_%s_library" % tag] = rec(timeit(lambda: torch.ops.aten.convolution_backward(
                dy, x, w, None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1, (False, True, False)), a.iters), flops)
            res["wgrad3x3_%s_kernel" % tag]["chunks"] = conv_wgrad_ext._lib().mdetr_conv_wgrad_chunks(B, H, W, C, H, W, C, 3, 1)

    # ---- stride-2 convolutions: forward, input gradient, weight gradient ----
    if a.only in ("", "strided"):
        shapes = (("layer2.0.conv2", 128, 128, 96, 320, 3), ("layer3.0.conv2", 256, 256, 48, 160, 3), ("layer4.0.conv2", 512, 512, 24, 80, 3),
                  ("input_proj.3", 2048, 256, 12, 40, 3), ("depth.downsample", 256, 256, 48, 160, 3),
                  ("layer2.0.downsample", 256, 512, 96, 320, 1), ("layer3.0.downsample", 512, 1024, 48, 160, 1), ("layer4.0.downsample", 1024, 2048, 24, 80, 1))
        for tag, C, N, H, W, k in shapes:
            x, w, dy, pad, flops = tensors(C, N, H, W, k, 2)
            sh = torch.randn(N, device=dev)
            shb = sh.to(torch.bfloat16)
            wo = conv_taps_ext._ohwi(w)
            res["fwd_%s_kernel" % tag] = rec(timeit(lambda: conv_taps_ext._forward(x, wo, sh, tag != "input_proj.3"), a.iters), flops)      # (the pyramid level has no ReLU: GroupNorm follows)
            res["fwd_%s_library" % tag] = rec(timeit(lambda: F.relu_(F.conv2d(x, w, shb, stride=2, padding=pad)), a.iters), flops)
            res["dgrad_%s_kernel" % tag] = rec(timeit(lambda: conv_taps_ext._input_gradient(dy, wo, H, W), a.iters), flops)
            res["dgrad_%s_library" % tag] = rec(timeit(lambda: torch.ops.aten.convolution_backward(
                dy, x, w, None, (2, 2), (pad, pad), (1, 1), False, (0, 0), 1, (True, False, False)), a.iters), flops)
            res["wgrad_%s_kernel" % tag] = rec(timeit(lambda: conv_wgrad_ext.weight_gradient(x, dy, k, 2, torch.bfloat16), a.iters), flops)
            res["wgrad_%s_library" % tag] = rec(timeit(lambda: torch.ops.aten.convolution_backward(
                dy, x, w, None, (2, 2), (pad, pad), (1, 1), False, (0, 0), 1, (False, True, False)), a.iters), flops)

    # ---- the stem: 7x7 / stride 2 / pad 3 on the 3-channel image (frozen: forward only) ----
    if a.only in ("", "stem"):
        try:
            from monodetr_amd import conv_stem_ext
            x = torch.randn(B, 3, 384, 1280, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            w = (torch.randn(64, 3, 7, 7, device=dev) / 12).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            sh = torch.randn(64, device=dev)
            shb = sh.to(torch.bfloat16)
            flops = 2.0 * B * 192 * 640 * 147 * 64
            packed = conv_stem_ext.pack_weight(w)
            res["stem_kernel"] = rec(timeit(lambda: conv_stem_ext._launch(x, packed, sh, True), a.iters), flops)
            res["stem_library"] = rec(timeit(lambda: F.relu_(F.conv2d(x, w, shb, stride=2, padding=3)), a.iters), flops)
        except ImportError:
            pass
    print(json.dumps(res))


if __name__ == "__main__":
    main()
