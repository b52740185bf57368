"""Deferred chunk sums (monodetr_amd/chunk_sums.py) under every gradient exchange the product offers, on the whole model with the
committed bf16 kernel list (MDETR_CHUNK_SUMS among it) and a ONE-RANK RCCL process group: the flat exchange and the two-part
(overlapped) one, launched eagerly and replayed from hipGraphs; the bucketed exchange and torch's DistributedDataParallel as
``bench.TrainStep`` wraps it (both eager-only).  Registered sums are filled with NaN until their flush (``chunk_sums.POISON``), so a
reader inside the backward pass -- a hook, DDP's reducer -- would leave NaN in the gradients it copied.

Each case against the gradients of the same seed and batch computed with every sum AT ONCE and no exchange (one rank: the average
is the gradient itself), over three consecutive iterations (dropout off, parameters held still): the same > 300 gradient tensors,
none non-finite, each within the spread two bf16 runs of this step have (2^-5 of the tensor's maximum, floor 1e-3 of the largest
gradient: the bar of tests/test_colsum_gpu.py), and the number of jobs that went through ``chunk_sums._launch``: the flat and the
two-part exchange must DEFER (as many jobs as the reference launched singly, in far fewer launches), the bucketed one and DDP read
inside the backward pass and must not (zero: every sum goes to the column-sum kernel at once).

One child process per case: the process group never outlives its case, and a capture never meets a live RCCL watchdog."""
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import monodetr_amd._runtime_env  # noqa: E402,F401  -- runtime flags, BEFORE torch loads the HIP runtime (the child process entry)

import pytest  # noqa: E402
import torch  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_faulted = []                            # a child that died of a signal or ran out of time: nothing more is started on the GPU


def _grads(step):
    torch.cuda.synchronize()
    return {n: p.grad.detach().float().clone() for n, p in step.raw_model.named_parameters() if p.grad is not None}


def _child(kind, launch, B):
    import bench
    from model_init import disable_dropout_
    from monodetr_amd import chunk_sums
    dev = torch.device("cuda", 0)
    names = tuple(sorted(bench.COMMITTED_SWITCHES["bf16"]))
    assert "MDETR_CHUNK_SUMS" in names
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29561")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sizes, real = [], chunk_sums._launch

    def counted(jobs):
        sizes.append(len(jobs))
        return real(jobs)

    def take():
        got = list(sizes)
        del sizes[:]
        return got

    def hold_still(step):
        """Gradients only: no optimizer step where the iteration is launched eagerly (as tests/test_colsum_gpu.py does); a replayed
        iteration keeps its captured optimizer graph and steps with a learning rate of zero instead."""
        disable_dropout_(step.raw_model)
        if launch == "eager":
            step.optimizer.step = lambda *a, **k: None
        else:
            for g in step.optimizer.param_groups:
                if torch.is_tensor(g["lr"]):
                    g["lr"].fill_(0.0)
                else:
                    g["lr"] = 0.0

    chunk_sums._launch = counted
    try:
        # the reference: every sum at once through the same kernel, no exchange
        chunk_sums.IMMEDIATE, chunk_sums.POISON = True, False
        ref = bench.TrainStep(dev, B, "bf16", size=(384, 1280), switches=names, graph=True)
        disable_dropout_(ref.raw_model)
        ref.optimizer.step = lambda *a, **k: None
        ref._eager(ref.inputs)
        want = _grads(ref)
        ref_sizes = take()
        del ref
        torch.cuda.empty_cache()
        chunk_sums.IMMEDIATE, chunk_sums.POISON = False, True
        per_iteration, got = [], []
        if launch == "graph":
            step = bench.TrainStep(dev, B, "bf16", size=(384, 1280), switches=names, graph=True, ddp=kind)
            hold_still(step)
            assert step.grad_sync is None and step.pending_sync == kind
            for _ in range(step.eager_steps):                # the warm-up iterations of a capture, launched eagerly
                step._eager(step.inputs)
            warm = take()
            step.capture()                                   # BEFORE the process group exists
            captured = take()                                # what the capture recorded: the same in every replay
            assert sum(warm) == step.eager_steps * sum(captured)
            torch.distributed.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
            mode = step.attach_process_group()
            assert step.graph is not None and step.grad_sync._static is not None, mode
            for _ in range(3):
                step()
                got.append(_grads(step))
                per_iteration.append(captured)
            assert step.replays == 3
        else:
            torch.distributed.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
            step = bench.TrainStep(dev, B, "bf16", size=(384, 1280), switches=names, graph=False, ddp=kind)
            hold_still(step)
            mode = "eager"
            for _ in range(3):
                step()
                got.append(_grads(step))
                per_iteration.append(take())
        wrapped = type(step.model).__name__
        sync = type(step.grad_sync).__name__
        floor = 1e-3 * max(float(t.abs().max()) for t in want.values())
        res = dict(kind=kind, launch=launch, B=B, mode=mode, wrapped=wrapped, sync=sync, n_ref=len(want), ref_jobs=sum(ref_sizes), ref_launches=len(ref_sizes),
                   same_set=[set(g) == set(want) for g in got],
                   nonfinite=[[n for n in g if not torch.isfinite(g[n]).all()][:6] for g in got],
                   worst=[max((float((want[n] - g[n]).abs().max() / want[n].abs().max().clamp_min(floor)), n) for n in want if n in g) for g in got],
                   jobs=[sum(s) for s in per_iteration], launches=[len(s) for s in per_iteration], largest=[max(s) if s else 0 for s in per_iteration])
        print("EXCHANGE-CHILD " + json.dumps(res), flush=True)
    finally:
        chunk_sums._launch = real
        chunk_sums.IMMEDIATE = chunk_sums.POISON = False
        if torch.distributed.is_initialized():
            torch.distributed.destroy_process_group()


@pytest.mark.parametrize("kind,launch,B,deferred", [
    ("flat", "eager", 2, True),
    ("flat", "graph", 8, True),              # the benchmarked geometry, the two-graph replay around the flat all-reduce
    ("overlap", "eager", 2, True),
    ("overlap", "graph", 2, True),           # three replays, the upper gradients' all-reduce beside the backbone's backward
    ("bucketed", "eager", 2, False),         # hooks read p.grad inside the backward pass: the deferral must be off
    ("ddp", "eager", 2, False),              # the reducer copies each gradient into its bucket as it arrives: off as well
])
def test_gradient_exchange_with_deferred_chunk_sums_gives_the_immediate_gradients(kind, launch, B, deferred):
    if _faulted:
        pytest.fail("not started: the case %s ended in a fault or ran out of time" % _faulted[0])
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([HERE, os.path.dirname(HERE)]))
    try:
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, launch, str(B)], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True, timeout=420)
    except subprocess.TimeoutExpired:
        _faulted.append((kind, launch))
        raise
    tail = done.stdout[-3000:]
    if done.returncode < 0 or done.returncode in (124, 134, 137, 139):
        _faulted.append((kind, launch))
    assert done.returncode == 0, tail
    res = json.loads([ln for ln in done.stdout.splitlines() if ln.startswith("EXCHANGE-CHILD ")][-1][len("EXCHANGE-CHILD "):])
    print(res)
    assert res["n_ref"] > 300 and res["same_set"] == [True] * 3, res
    assert res["nonfinite"] == [[], [], []], res
    assert all(w[0] <= 2.0 ** -5 for w in res["worst"]), res["worst"]
    assert res["wrapped"] == ("DistributedDataParallel" if kind == "ddp" else "MonoDETR")
    assert res["sync"] == {"flat": "FlatGradSync", "overlap": "SplitGradSync", "bucketed": "BucketedGradSync", "ddp": "NoneType"}[kind]
    if launch == "graph":
        assert res["mode"].startswith("three hipGraph replays" if kind == "overlap" else "two hipGraph replays"), res["mode"]
    # the reference launched every sum singly through the same entry: that many sums exist in a backward pass of this model
    assert res["ref_jobs"] == res["ref_launches"] > 1, res
    if deferred:
        # every one of them registered, and computed by fewer launches, one of them at least a flush of several jobs
        assert res["jobs"] == [res["ref_jobs"]] * 3 and all(n < res["ref_jobs"] for n in res["launches"]) and min(res["largest"]) > 1, res
    else:
        assert res["jobs"] == [0, 0, 0], res


if __name__ == "__main__":
    if "--child" in sys.argv:
        i = sys.argv.index("--child")
        _child(sys.argv[i + 1], sys.argv[i + 2], int(sys.argv[i + 3]))
