"""A small stack of the product's own layers on the emulated kernels, driven by the product's ``TrainIteration`` -- the harness of
tests/test_deferred_sums_emulated_cpu.py and of the world-2 run of tests/test_ddp_cpu.py (test infrastructure).

  image [2, 64, 8, 16] -> Conv3x3 (bias) -> ReLU -> ConvStrided 3x3 / 2 (bias)           "backbone": below ``pyramid``'s cut
  tokens [1, 1152, 64] + the level's channel means -> 3 x linear.Linear (bias), ReLU in between       the part above the cut

Every weight gradient comes from a split kernel (csrc/conv_wgrad.hip, csrc/twgrad.hip) whose chunk sums go through
``chunk_sums.chunk_sum``: 2 / 4 / 9 chunks here.  ``run_case`` runs iterations under one CONSUMER of the gradients and returns what
each iteration left in ``.grad``, the operands and results of every weight-gradient call, and what reached ``chunk_sums``."""
import contextlib

import torch

T, CH = 1152, 64
LINEARS = 3
SUMS = LINEARS + 2                   # chunk sums per backward pass: one per weight gradient


class Interrupted(RuntimeError):
    pass


def _interrupt(grad):
    raise Interrupted("stop")


class Stack(torch.nn.Module):
    def __init__(self, nchw_weight=False):
        super().__init__()
        self.interrupt = False                            # raise `Interrupted` in the backward pass between lins[1] and lins[0]
        from monodetr_amd import conv3x3_ext, conv_taps_ext
        from monodetr_amd.monodetr import linear
        g = torch.Generator().manual_seed(5)
        self.conv = conv3x3_ext.Conv3x3(CH, CH, kernel_size=(3, 3), padding=1)
        self.down = conv_taps_ext.ConvStrided(CH, CH, kernel_size=(3, 3), stride=2, padding=1)
        self.lins = torch.nn.ModuleList(linear.Linear(CH, CH) for _ in range(LINEARS))
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * (0.1 if p.dim() > 1 else 0.05))
        self.to(torch.bfloat16).to(memory_format=torch.channels_last)
        if nchw_weight:                                   # the parameter NCHW-contiguous, the kernel's gradient channels_last
            self.conv.weight.data = self.conv.weight.data.contiguous()

    def pyramid(self, image):
        f = self.down(torch.relu(self.conv(image)))
        boundary = self.__dict__.get("_grad_boundary")    # (the protocol of MonoDETR.pyramid: TrainIteration's cut backward pass)
        if boundary is not None and torch.is_grad_enabled():
            fd = f.detach().requires_grad_(True)
            boundary.append((f, fd))
            f = fd
        return f

    def forward(self, image, tokens):
        f = self.pyramid(image)
        h = tokens + f.float().mean((0, 2, 3)).to(tokens.dtype)
        for i, lin in enumerate(self.lins):
            h = lin(h)
            if i + 1 < len(self.lins):
                h = torch.relu(h)
            if i == 0 and self.interrupt:
                h.register_hook(_interrupt)
        return h


def batch(seed):
    g = torch.Generator().manual_seed(seed)
    image = torch.randn(2, CH, 8, 16, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    tokens = (torch.randn(1, T, CH, generator=g) * 0.5).to(torch.bfloat16)
    proj = (torch.randn(1, T, CH, generator=g) * 0.1).to(torch.bfloat16)
    return image, tokens, proj


class NoOptimizer:
    """Gradients only.  keep: ``zero_grad`` leaves ``.grad`` in place (gradient accumulation over several backward passes)."""

    def __init__(self, params, keep=False):
        self.params, self.keep = list(params), keep

    def zero_grad(self, set_to_none=True):
        if not self.keep:
            for p in self.params:
                p.grad = None

    def step(self):
        pass


@contextlib.contextmanager
def emulated(mode):
    """The kernels of the stack on the HIP-on-CPU shim, chunk sums on; mode "deferred": batched, registered results poisoned until
    their flush; "immediate": every sum at once through the same kernel.  Everything is put back afterwards."""
    import native_emul
    from monodetr_amd import bias_act_ext, chunk_sums, conv3x3_ext, conv_taps_ext, conv_wgrad_ext, small_wgrad_ext, tgemm_ext
    from monodetr_amd.monodetr import linear
    L = native_emul.lib()
    mods = (chunk_sums, conv3x3_ext, conv_taps_ext, conv_wgrad_ext, tgemm_ext, bias_act_ext)
    saved = [(m, "_backend", m._backend) for m in mods] + [(m, "ENABLED", m.ENABLED) for m in (chunk_sums, conv3x3_ext, conv_taps_ext, small_wgrad_ext)] + \
        [(chunk_sums, "POISON", chunk_sums.POISON), (chunk_sums, "IMMEDIATE", chunk_sums.IMMEDIATE), (linear, "_TGEMM", linear._TGEMM),
         (linear, "_MIN_TOKENS", linear._MIN_TOKENS)]
    try:
        for m in mods:
            m._backend = L
        chunk_sums.ENABLED = conv3x3_ext.ENABLED = conv_taps_ext.ENABLED = linear._TGEMM = True
        small_wgrad_ext.ENABLED = False
        linear._MIN_TOKENS = 1024                         # (the 1 152 token rows of this stack take the kernels' route)
        chunk_sums.POISON, chunk_sums.IMMEDIATE = mode == "deferred", mode == "immediate"
        yield L
    finally:
        for m, name, v in saved:
            setattr(m, name, v)


class Probe:
    """What reaches chunk_sums (registrations, jobs per launch) and every weight-gradient call (operands, results -- as detached
    aliases: a second reference to the result itself would keep AccumulateGrad from taking it over, and the copy it then makes is
    a read before the flush)."""

    def __init__(self):
        self.registered, self.launches, self.calls = 0, [], []

    def __enter__(self):
        from monodetr_amd import chunk_sums, conv_wgrad_ext
        self._saved = (chunk_sums._launch, chunk_sums.chunk_sum, conv_wgrad_ext.token_weight_gradient, conv_wgrad_ext.weight_gradient)
        launch, chunk_sum, token, conv = self._saved

        def _launch(jobs):
            self.launches.append(len(jobs))
            return launch(jobs)

        def _chunk_sum(*a, **kw):
            before = len(chunk_sums._pending)
            out = chunk_sum(*a, **kw)
            self.registered += len(chunk_sums._pending) - before
            return out

        def _token(x2, dy2, dtype, bias=False):
            dw, db = token(x2, dy2, dtype, bias=bias)
            self.calls.append(("token", x2.detach().clone(), dy2.detach().clone(), dw.detach(), db.detach(), conv_wgrad_ext._lib().mdetr_token_wgrad_chunks(
                x2.shape[0], x2.shape[1], dy2.shape[1])))
            return dw, db

        def _conv(x, dy, k, stride, dtype=torch.bfloat16, **kw):
            dw = conv(x, dy, k, stride, dtype, **kw)
            B, C, H, W = x.shape
            self.calls.append(("conv", x.detach().clone(), dy.detach().clone(), dw.detach(), (k, stride), conv_wgrad_ext._lib().mdetr_conv_wgrad_chunks(
                B, H, W, C, dy.shape[2], dy.shape[3], dy.shape[1], k, stride)))
            return dw

        chunk_sums._launch, chunk_sums.chunk_sum, conv_wgrad_ext.token_weight_gradient, conv_wgrad_ext.weight_gradient = _launch, _chunk_sum, _token, _conv
        return self

    def __exit__(self, *exc):
        from monodetr_amd import chunk_sums, conv_wgrad_ext
        chunk_sums._launch, chunk_sums.chunk_sum, conv_wgrad_ext.token_weight_gradient, conv_wgrad_ext.weight_gradient = self._saved
        return False

    def take(self):
        # (copies, taken once the iteration is over: a later backward pass may add into a tensor that became a .grad)
        calls = [tuple(v.clone() if torch.is_tensor(v) else v for v in c) for c in self.calls]
        got = dict(registered=self.registered, launches=self.launches, calls=calls)
        self.registered, self.launches, self.calls = 0, [], []
        return got




def make_iteration(consumer, model):
    """The product's TrainIteration on the stack with one consumer of the gradients attached -> (iteration, notes)."""
    from monodetr_amd.helpers.dist_helper import BucketedGradSync, FlatGradSync, SplitGradSync
    from monodetr_amd.helpers.step_helper import TrainIteration
    notes = {"hook_saw": []}
    sync = {"flat": FlatGradSync, "split": SplitGradSync}.get(consumer)
    sync = sync(model.parameters()) if sync else (BucketedGradSync(model.parameters(), bucket_mb=0.006) if consumer == "bucketed" else None)
    it = TrainIteration(model, None, NoOptimizer(model.parameters(), keep=consumer == "retained"), torch.device("cpu"), grad_sync=sync,
                        compute=lambda b: ((it.model(b[0], b[1]).float() * b[2].float()).sum() * 0.01, {}))
    if consumer in ("ddp_view", "ddp_copy"):
        from torch.nn.parallel import DistributedDataParallel as DDP
        it.model = DDP(model, static_graph=True, gradient_as_bucket_view=consumer == "ddp_view", bucket_cap_mb=0.006)     # (as bench.TrainStep wraps it)
    if consumer == "hooks":
        model.lins[1].weight.register_hook(lambda g: g * 1)
        model.lins[0].weight.register_post_accumulate_grad_hook(lambda p: notes["hook_saw"].append(p.grad.detach().clone()))
    return it, notes


def run_case(consumer, mode, iters=3, seed0=40):
    """`iters` iterations of the stack under `consumer` -> [per iteration: {name: gradient}], [per iteration: Probe.take()], notes."""
    with emulated(mode), Probe() as probe:
        model = Stack(nchw_weight=consumer == "nchw_weight")
        it, notes = make_iteration(consumer, model)
        notes["route"] = type(model.pyramid(batch(0)[0]).grad_fn).__name__
        notes["conv_route"] = type(model.conv(batch(0)[0]).grad_fn).__name__
        grads, seen = [], []
        for i in range(iters):
            it._step(batch(seed0 + i))
            grads.append({n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})
            seen.append(probe.take())
        notes["grad_strides"] = {n: tuple(p.grad.stride()) for n, p in model.named_parameters() if p.grad is not None}
        notes["buckets"] = len(it.grad_sync.buckets) if consumer == "bucketed" else None
        return grads, seen, notes
