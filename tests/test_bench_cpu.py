"""Host logic of bench.py that needs no GPU: `python bench.py --gpus N` outside torchrun starts its N ranks itself."""
import subprocess
import sys

import pytest

import bench


def test_plain_invocation_with_several_gpus_reexecutes_under_torchrun(monkeypatch):
    seen = {}

    def fake_call(cmd, env=None, cwd=None):
        seen.update(cmd=cmd, env=env, cwd=cwd)
        return 7

    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "5", "--warmup", "2"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 7                                            # the launcher's status is passed through
    cmd = seen["cmd"]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    assert cmd[-6:] == ["--gpus", "4", "--steps", "5", "--warmup", "2"] and cmd[-7].endswith("bench.py")
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_a_mismatched_world_size_is_refused(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert "does not match" in str(e.value.code)


def test_traffic_record_is_tied_to_the_kernel_source(tmp_path):
    import json
    p = str(tmp_path / "t.json")
    json.dump({"kernel_source_sha": "0" * 16, "msda_backward_bf16_Lq10200": 1}, open(p, "w"))
    rec, note = bench.pmc_traffic(p)
    assert rec == {} and "another kernel source" in note               # never a stale figure
    json.dump({"kernel_source_sha": bench.kernel_source_sha(), "msda_backward_bf16_Lq10200": 5, "source": "profiles/x.json"}, open(p, "w"))
    rec, note = bench.pmc_traffic(p)
    assert rec["msda_backward_bf16_Lq10200"] == 5 and note == "profiles/x.json"


def test_families_table_groups_kernels_and_prices_them_against_their_bound():
    """bench.families_table: kernels -> families by name, declared work -> bound (HBM 8 TB/s vs bf16 MFMA 2.5 PFLOP/s, the slower one)
    and the fraction of it reached; families without declared work carry their time only."""
    import bench
    rows = [("void mdetr::(anonymous namespace)::tgemm_kernel<128, 128, false, 2, 0>(mdetr::TgemmArgs)", 20, 500.0),
            ("void mdetr::(anonymous namespace)::twgrad_kernel<128, 128, 32, 2>(mdetr::TwgradArgs)", 4, 100.0),
            ("void mdetr::(anonymous namespace)::conv_wgrad_kernel<1, 3>(x)", 2, 80.0),
            ("Cijk_Ailk_Bljk_BBS", 10, 200.0), ("void at::native::vectorized_elementwise_kernel<8, x>", 40, 160.0),
            ("void mdetr::(anonymous namespace)::msda_bwd_fused<a>", 6, 2800.0), ("something_else", 2, 10.0)]
    t = {r["name"]: r for r in bench.families_table(rows, {10: (214000.0, 1680000.0), 11: (42800.0, 400000.0), 9: (36000.0, 20000.0)}, msda_bytes=2.5e9,
                                                    attn_flop=0.0, iterations=2)}
    assert t["token_gemm"]["launches"] == 10 and t["token_gemm"]["ms_per_step"] == 0.25
    assert t["token_gemm"]["bound"] == "hbm" and abs(t["token_gemm"]["frac"] - (0.84e9 / 8e12) / 0.25e-3) < 1e-3
    assert t["token_weight_gradient"]["launches"] == 2 and t["convolutions"]["bound"] == "mfma"
    assert t["msda"]["algorithmic_bytes"] == 2500000000 and t["msda"]["bound"] == "hbm"
    assert t["library_gemm"]["frac"] is None and t["framework_elementwise"]["launches"] == 20 and "other" in t
    assert bench.family_of("void mdetr::(anonymous namespace)::conv_wgrad_kernel<1, 1>(x)") == "token_weight_gradient"


def _mock_gpu(monkeypatch, Step):
    """bench.main() with the GPU mocked away and `Step` standing in for the training iteration."""
    import contextlib
    import torch
    from monodetr_amd import _capi

    def no_topology(i):
        raise AttributeError
    enabled = []
    for k in [k for k in __import__("os").environ if k.startswith("MDETR_")]:
        monkeypatch.delenv(k)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.setattr(torch.cuda, "empty_cache", lambda: None)
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "get_device_properties", no_topology)
    monkeypatch.setattr(_capi, "lib", lambda: None)
    monkeypatch.setattr(_capi, "profile_enable", lambda on: enabled.append(on))
    monkeypatch.setattr(_capi, "profile_read", lambda: pytest.fail("a plain run reads no per-kernel timings"))
    monkeypatch.setattr(_capi, "profile_read_work", lambda: pytest.fail("a plain run reads no per-kernel work"))
    monkeypatch.setattr(bench, "TrainStep", Step)
    monkeypatch.setattr(bench, "gpu_clocks", lambda i=0: pytest.fail("a plain run does not query the clocks"))
    monkeypatch.setattr(bench, "cpu_baseline", lambda *a: pytest.fail("a plain run has no CPU baseline"))
    return enabled


class _FakeStep:
    """A stand-in training iteration: a tiny model whose parameters every call moves, a loss that counts the calls since the
    initial state; `log` records the calls and the state restores in order."""
    built = []

    def __init__(self, *a, switches=None, **k):
        import torch
        torch.manual_seed(0)
        self.switches = set(switches or [])
        self.raw_model = torch.nn.Sequential(torch.nn.Linear(300, 40), torch.nn.Linear(40, 3), torch.nn.Linear(3, 1, bias=False))
        self.raw_model[1].bias.requires_grad_(False)
        self.calls, self.eager, self.n, self.log = 0, 0, 0, []
        self.graph = self.stream = None
        _FakeStep.built.append(k)

    def try_capture(self):
        self.graph = object()
        return "one hipGraph replay per iteration"

    def remember_initial_state(self):
        self.log.append("remember")
        self._initial = [p.detach().clone() for p in self.raw_model.parameters()]

    def restore_initial_state(self):
        import torch
        self.log.append("restore")
        with torch.no_grad():
            for p, p0 in zip(self.raw_model.parameters(), self._initial):
                p.copy_(p0)
        self.n = 0

    def __call__(self):
        import torch
        self.calls += 1
        self.n += 1
        self.log.append("call")
        with torch.no_grad():
            for p in self.raw_model.parameters():
                if p.requires_grad:
                    p.grad = torch.full_like(p, 0.5 * self.n)
                    p.add_(p.grad, alpha=-0.01)
        self.losses = {"loss_ce": torch.tensor(0.25 * self.n), "loss_bbox_0": torch.tensor([1.0 + self.n]), "class_error": 12.5}
        return torch.tensor(2.0 * self.n, requires_grad=True)

    def eager_iteration(self):
        self.eager += 1
        self.log.append("eager")
        return self()


def _run(monkeypatch, capsys, argv):
    import json
    del _FakeStep.built[:]
    steps = []
    orig = _FakeStep.__init__

    def init(self, *a, **k):
        orig(self, *a, **k)
        steps.append(self)
    monkeypatch.setattr(_FakeStep, "__init__", init)
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    bench.main()
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1]), steps


def test_a_plain_run_times_the_steps_and_measures_nothing_else(monkeypatch, capsys):
    """`bench.py --gpus 1 --steps N --warmup W`: one step built, prime + W + N calls of it and nothing more -- no per-kernel
    events, no eager iterations, no side measurements, no CPU baseline -- and the headline keys of the line."""
    enabled = _mock_gpu(monkeypatch, _FakeStep)
    line, steps = _run(monkeypatch, capsys, ["--gpus", "1", "--steps", "7", "--warmup", "3", "--prime", "2"])
    assert len(steps) == 1 and steps[0].calls == 2 + 3 + 7 and steps[0].eager == 0 and not any(enabled)
    assert line["steps"] == 7 and line["warmup"] == 3 and line["n_gpus"] == 1 and line["higher_is_better"] is True
    assert line["metric"].startswith("training images/sec") and line["unit"] == "images/sec" and line["dtype"] == "bf16"
    assert line["value"] > 0 and abs(line["value"] - 8 * 1e3 / line["ms_per_step"]) <= 1e-2 * line["value"]
    assert line["final_loss"] == 2.0 * 12 and line["config"]["launch"].startswith("one hipGraph replay")
    for k in ("roofline", "kernels", "mfma", "families", "fp32_path", "eager_path", "default_path", "config2", "config5",
              "rccl_1rank", "cpu_baseline"):
        assert k not in line, k
    with pytest.raises(SystemExit):
        _run(monkeypatch, capsys, ["--steps", "0"])


def test_dump_outputs_writes_one_more_iteration_of_the_timed_step_from_its_initial_state(monkeypatch, capsys, tmp_path):
    """--dump-outputs DIR: the timed step itself -- its initial state remembered before its first iteration, restored after
    the timed steps -- runs once more the way it was timed, before anything else (--full's extras follow), and its loss, the
    criterion's entries and its sampled parameters / gradients are written as float32; the files do not depend on how many
    steps were timed."""
    import numpy as np
    import torch
    _mock_gpu(monkeypatch, _FakeStep)
    monkeypatch.setattr(bench, "DUMP_PER_TENSOR", 128)
    outs = []
    for i, extra in enumerate(([], ["--full", "--no-variants", "--no-cpu-baseline"], ["--steps", "9", "--warmup", "3"])):
        d = tmp_path / ("run%d" % i)
        monkeypatch.setattr(bench, "profile_kernels", lambda step, n: [])
        if "--full" in extra:
            from monodetr_amd import _capi
            monkeypatch.setattr(_capi, "profile_read", lambda: [])
            monkeypatch.setattr(_capi, "profile_read_work", lambda: [])
            monkeypatch.setattr(bench, "gpu_clocks", lambda i=0: None)
        line, steps = _run(monkeypatch, capsys, ["--steps", "4", "--warmup", "1", "--prime", "1", "--dump-outputs", str(d)] + extra)
        timed = steps[0]
        n = 1 + (3 if "--warmup" in extra else 1) + (9 if "--steps" in extra else 4)
        assert len(steps) == 1 and timed.log[:n + 3] == ["remember"] + ["call"] * n + ["restore", "call"]
        assert line["steps"] == (9 if "--steps" in extra else 4)
        files = {f.name[:-4]: np.load(str(f)) for f in d.iterdir()}
        assert set(files) == {"loss", "parameters", "gradients", "loss_ce", "loss_bbox_0", "class_error"}
        assert all(a.dtype == np.float32 for a in files.values())
        assert files["loss"] == 2.0 and files["loss_ce"] == 0.25 and files["class_error"] == 12.5
        assert files["loss_bbox_0"].tolist() == [2.0]
        # parameters in named_parameters() order: 128 sampled positions of the 12 000-element weight, all of the smaller tensors
        assert files["parameters"].shape == files["gradients"].shape == (128 + 40 + 120 + 3 + 3,)
        if not extra:
            model = timed.raw_model                                   # (nothing ran after the dumped iteration)
            assert np.array_equal(files["parameters"][128:168], model[0].bias.detach().numpy())
            assert np.array_equal(files["parameters"][-3:], model[2].weight.detach().numpy().ravel())
            gen = torch.Generator().manual_seed(0)
            idx = torch.randint(0, 12000, (128,), generator=gen)
            assert np.array_equal(files["parameters"][:128], model[0].weight.detach().reshape(-1)[idx].numpy())
        assert np.all(files["gradients"][128 + 40 + 120:-3] == 0) and np.all(files["gradients"][:128] == 0.5)
        outs.append(files)
    for other in outs[1:]:                                            # whatever the timed steps did: the same files
        assert all(np.array_equal(outs[0][k], other[k]) for k in outs[0])
    with pytest.raises(SystemExit):
        _run(monkeypatch, capsys, ["--gpus", "2", "--dump-outputs", str(tmp_path / "x")])


@pytest.mark.parametrize("fused", [False, True], ids=["adamw", "fused_adamw"])
def test_restore_initial_state_repeats_the_first_iteration(fused):
    """TrainStep.restore_initial_state with the project's optimizers (capturable: device step counters; a bf16 layer: fp32
    master copies; the fused form: flat buffers): after a few iterations, the restored state's next iteration is the first
    one again, bit for bit."""
    import types
    import torch
    import backends
    from monodetr_amd.helpers.optimizer_helper import AdamW, FusedAdamW
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Linear(16, 4).to(torch.bfloat16))
    groups = [{"params": [p for k, p in model.named_parameters() if "bias" in k], "weight_decay": 0},
              {"params": [p for k, p in model.named_parameters() if "bias" not in k], "weight_decay": 1e-4}]
    opt = (FusedAdamW if fused else AdamW)(groups, lr=1e-2, capturable=True)
    if fused:
        opt._lib, opt._allow_cpu = backends.get("host"), True
    x = torch.randn(32, 8)

    def iteration():
        opt.zero_grad(set_to_none=True)
        loss = model[1](model[0](x).to(torch.bfloat16)).float().square().mean()
        loss.backward()
        opt.step()
        return [loss.detach()] + [p.detach().clone() for p in model.parameters()]
    step = types.SimpleNamespace(raw_model=model, optimizer=opt)
    bench.TrainStep.remember_initial_state(step)
    first = iteration()
    later = [iteration() for _ in range(3)]
    assert not torch.equal(later[-1][1], first[1])
    bench.TrainStep.restore_initial_state(step)
    again = iteration()
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert all(torch.equal(a, b) for a, b in zip(later[0], iteration()))          # ... and the second one after it
