"""mdetr_token_wgrad_grouped on the device: the job lists of tests/twgrad_grouped_cases.py (as tests/test_twgrad_grouped_emulated_cpu.py
runs them on the shim), and two modules whose backward pass runs under ``chunk_sums.deferred()`` with the family MDETR_TWGRAD_GROUPED on
and off -- every parameter gradient ``torch.equal`` between the two, registered results poisoned until their flush (POISON) and every
registered operand compared with its clone at the flush (VERIFY)."""
import contextlib

import pytest
import torch

import twgrad_grouped_cases as G
from conftest import tune

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def lib():
    from monodetr_amd import _capi
    return _capi.lib()


@pytest.fixture
def plain(monkeypatch):
    tune(monkeypatch, twgrad=None, twgrad_kg=None, twgrad_wgs=None)


@pytest.mark.parametrize("kind", ["ints", "randn"])
def test_grouped_every_shape_equals_the_single_launches(lib, plain, kind):
    G.check(lib, dev(), G.ALL_SHAPES, kind, want_dead=True)
    G.check(lib, dev(), G.ALL_SHAPES_OTHER_BIAS, kind)


def test_grouped_mixed_instantiations_in_one_call(lib, plain):
    G.check(lib, dev(), G.MIXED, "ints")
    G.check(lib, dev(), G.MIXED, "randn")


def test_grouped_one_job_more_than_a_launch_holds(lib, plain):
    G.check(lib, dev(), G.ONE_MORE_THAN_THE_CAP, "ints", want_dead=True)
    G.check(lib, dev(), G.ONE_MORE_THAN_THE_CAP, "randn", want_dead=True)


def test_grouped_dead_workgroups_between_jobs(lib, plain):
    G.check(lib, dev(), G.DEAD_WORKGROUPS, "ints", want_dead=True)
    G.check(lib, dev(), G.DEAD_WORKGROUPS, "randn", want_dead=True)


def test_grouped_two_wave_groups(lib, monkeypatch):
    tune(monkeypatch, twgrad=None, twgrad_kg="2", twgrad_wgs=None)
    G.check(lib, dev(), G.TWO_WAVE_GROUPS, "ints")
    G.check(lib, dev(), G.TWO_WAVE_GROUPS, "randn")


def test_grouped_validation_errors(lib, plain):
    G.check_validation(lib, dev())


# ---- modules: the backward pass under deferred(), family on and off ---------------------------------------------------------------
@contextlib.contextmanager
def committed(family_on, monkeypatch):
    """The committed bf16 families with / without MDETR_TWGRAD_GROUPED; POISON and VERIFY on; the kernels' routes from 1 024 token rows
    on (the step's 4 400-row layers take them; these modules run 1 100 rows).  -> the registered producers, counted."""
    import bench
    from monodetr_amd import chunk_sums
    from monodetr_amd.monodetr import linear
    names = set(bench.COMMITTED_SWITCHES["bf16"]) - {"MDETR_TWGRAD_GROUPED"}
    bench.apply_switches(names | ({"MDETR_TWGRAD_GROUPED"} if family_on else set()))
    monkeypatch.setattr(linear, "_MIN_TOKENS", 1024)
    monkeypatch.setattr(chunk_sums, "POISON", True)
    monkeypatch.setattr(chunk_sums, "VERIFY", True)
    count = [0]
    register = chunk_sums.register_producer
    monkeypatch.setattr(chunk_sums, "register_producer", lambda *a: (count.__setitem__(0, count[0] + 1), register(*a))[1])
    try:
        yield count
    finally:
        monkeypatch.undo()
        bench.apply_switches(set())


def rand(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(torch.bfloat16).to(dev())


def both_ways(build, run, monkeypatch, at_least):
    """build() -> module (the same weights both times); run(module) -> [outputs].  -> the gradients of the family-on run, after the
    comparison with the family-off run."""
    from monodetr_amd import chunk_sums
    res = {}
    for on in (False, True):
        with committed(on, monkeypatch) as count:
            torch.manual_seed(11)
            module = build().to(torch.bfloat16).to(dev()).train()
            with torch.no_grad():
                for i, p in enumerate(module.parameters()):
                    p.copy_(rand(*p.shape, seed=100 + i, scale=0.05 if p.dim() > 1 else 0.5))
            outs = run(module)
            with chunk_sums.deferred(params=list(module.parameters())) as d:
                assert d.reason is None
                torch.autograd.backward(outs, [rand(*o.shape, seed=7 + k) for k, o in enumerate(outs)])
            assert not chunk_sums._producers and not chunk_sums._pending
            assert (count[0] >= at_least) if on else (count[0] == 0), count[0]
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


def test_grouped_two_layer_token_mlp_gradients_equal_the_family_off_run(monkeypatch):
    from monodetr_amd.monodetr import linear

    class MLP(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b = linear.Linear(256, 136), linear.Linear(136, 72)

        def forward(self, x):
            return self.b(torch.relu(self.a(x)))

    x = rand(1, 1100, 256, seed=1).requires_grad_(True)
    g = both_ways(MLP, lambda m: [m(x)], monkeypatch, at_least=2)
    assert all(v is not None and float(v.float().abs().max()) > 0 for v in g.values()) and len(g) == 4


def test_grouped_decoder_layer_gradients_equal_the_family_off_run(monkeypatch):
    """One decoder layer in the smallest configuration of the module tests (tests/test_wpack_gpu.py: d_model 256, d_ffn 64, four tiny
    levels, two query groups), with 2 x 550 = 1 100 query rows: its projections and FFN are the step's 4 400-row class."""
    from monodetr_amd.monodetr.depthaware_transformer import DepthAwareDecoderLayer
    levels = [(3, 5), (2, 3), (1, 2), (1, 1)]
    S = sum(h * w for h, w in levels)
    shapes = torch.tensor(levels, dtype=torch.long, device=dev())
    starts = torch.cat((shapes.new_zeros((1,)), shapes.prod(1).cumsum(0)[:-1]))
    tgt, qpos = rand(2, 550, 256, seed=1).requires_grad_(True), rand(2, 550, 256, seed=2)
    memory, depth = rand(2, S, 256, seed=3).requires_grad_(True), rand(5, 2, 256, seed=4)
    ref = (0.2 + 0.6 * torch.rand(2, 550, 1, 6, generator=torch.Generator().manual_seed(5))).expand(-1, -1, len(levels), -1).to(dev())
    g = both_ways(lambda: DepthAwareDecoderLayer(256, 64, 0.0, "relu", len(levels), 8, 4, group_num=2),
                  lambda m: [m(tgt, qpos, ref, memory, shapes, starts, None, depth, None, 2)], monkeypatch, at_least=4)
    assert g["linear1.weight"] is not None and g["linear2.weight"] is not None
