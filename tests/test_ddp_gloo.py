"""CPU, world_size 2, gloo: the N>1 path of the step -- ONE all-reduce (sum) of the flat gradient buffer, then the
1/world scale folded into the optimiser -- reproduces single-process gradients of the concatenated batch."""
import os

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fal_net_amd import train


class _FlatModel:
    """Stand-in exposing the two accessors train.allreduce_gradients uses (the real module needs a GPU)."""

    def __init__(self, n):
        self.g = torch.zeros(n)

    def flat_gradients(self):
        return self.g


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(0)
    w = torch.randn(16, 5)
    x = torch.randn(world * 4, 16, generator=torch.Generator().manual_seed(1))
    shard = x[rank * 4:(rank + 1) * 4]
    wl = w.clone().requires_grad_(True)
    (shard @ wl).pow(2).mean().backward()  # local mean loss on this rank's shard of the batch
    m = _FlatModel(wl.numel())
    m.g.copy_(wl.grad.reshape(-1))
    scale = train.allreduce_gradients(m)
    if rank == 0:
        torch.save({"g": m.g * scale, "scale": scale}, out)
    dist.destroy_process_group()


def test_allreduce_of_flat_gradients_equals_big_batch(tmp_path):
    world, out = 2, str(tmp_path / "r0.pt")
    mp.spawn(_worker, args=(world, 29533, out), nprocs=world, join=True)
    got = torch.load(out)
    assert abs(got["scale"] - 0.5) < 1e-12
    torch.manual_seed(0)
    w = torch.randn(16, 5, requires_grad=True)
    x = torch.randn(world * 4, 16, generator=torch.Generator().manual_seed(1))
    (x @ w).pow(2).mean().backward()
    assert torch.allclose(got["g"], w.grad.reshape(-1), atol=1e-6)


def test_single_process_is_identity():
    m = _FlatModel(8)
    m.g.fill_(3.0)
    assert train.allreduce_gradients(m) == 1.0 and float(m.g.sum()) == 24.0


def _worker_buckets(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    n = 1000
    m = _FlatModel(n)
    m.g.copy_(torch.arange(n, dtype=torch.float32) * (rank + 1))
    train.enable_overlapped_allreduce(m)
    assert m.bucket_hook is not None
    # backward finalises contiguous ranges of the flat buffer back to front (FAL_net.gradient_buckets): one async all-reduce each
    for i, (lo, hi) in enumerate([(700, n), (300, 700), (10, 300), (0, 10)]):
        m.bucket_hook(i, m.g[lo:hi])
    scale = train.allreduce_gradients(m)  # waits for the pending bucket reductions; no second collective
    if rank == 0:
        torch.save({"g": m.g.clone(), "scale": scale, "pending": len(m._pending_reduces)}, out)
    dist.destroy_process_group()


def test_bucketed_allreduce_covers_the_flat_buffer_once(tmp_path):
    world, out = 2, str(tmp_path / "r0b.pt")
    mp.spawn(_worker_buckets, args=(world, 29534, out), nprocs=world, join=True)
    got = torch.load(out)
    assert got["scale"] == 0.5 and got["pending"] == 0
    assert torch.equal(got["g"], torch.arange(1000, dtype=torch.float32) * 3)  # rank0 (x1) + rank1 (x2), every element exactly once


# ---- the REAL module on CPU: flat parameter / gradient buffers and their bucket ranges need no GPU (FAL_net.ensure_flat) ----
def _real_model(arch, levels=7, seed=0):
    from fal_net_amd import models as M
    torch.manual_seed(seed)
    return getattr(M, "FAL_net" + arch)(None, no_levels=levels)


def test_gradient_buckets_of_the_real_models_tile_the_flat_buffer():
    """FAL_netB / A / C: gradient_buckets() are contiguous, disjoint, cover [0, total) and come in the order backward finalises
    them (decoder + logits conv, encoder levels 4-6, 2-3, 0-1); every trainable parameter lies inside exactly one bucket."""
    for arch in ("B", "A", "C"):
        m = _real_model(arch)
        flat = m.ensure_flat("cpu")
        buckets = m.gradient_buckets()
        total = flat.numel()
        assert len(buckets) == 4 and buckets[0][1] == total and buckets[-1][0] == 0
        for (lo, hi), (lo2, hi2) in zip(buckets[:-1], buckets[1:]):
            assert lo < hi and hi2 == lo  # back to front, touching, no overlap
        named = m._trainable_named()
        pre = "backbone." if arch == "B" else ("BackBone." if arch == "A" else "synth.")
        want = {0: ("deconv", "iconv", "conv0."), 1: ("conv4", "conv5", "conv6"), 2: ("conv2", "conv3"), 3: ("conv0", "conv1")}
        for (n, p), off in zip(named, m._offsets):
            inside = [i for i, (lo, hi) in enumerate(buckets) if lo <= off and off + p.numel() <= hi]
            assert len(inside) == 1, (arch, n)
            short = n[len(pre):] if n.startswith(pre) else n
            assert short.startswith(want[inside[0]]), (arch, n, inside[0])
        assert all("amask_conv" not in n for n, _ in named)


def _worker_real(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    m = _real_model("B", seed=100 + rank)  # every rank starts from DIFFERENT random weights ...
    before = m.ensure_flat("cpu").clone()
    assert train.sync_parameters(m)        # ... and holds rank 0's after the start-up broadcast
    flat = m.flat_parameters()
    g = m.flat_gradients()
    g.copy_(torch.arange(g.numel(), dtype=torch.float32) % 97 * (rank + 1))
    train.enable_overlapped_allreduce(m)
    for i in range(4):                     # backward finalises the four real buckets in this order
        m._bucket_ready(i)
    n_async = len(m._pending_reduces)
    scale = train.allreduce_gradients(m)
    # an accumulating backward must not fire the per-bucket all-reduce again (the running sum would be reduced twice)
    m._accumulating = True
    m._bucket_ready(0)
    n_acc = len(m._pending_reduces)
    if rank == 0:
        torch.save({"flat": flat.clone(), "g": g.clone(), "scale": scale, "n_async": n_async, "n_acc": n_acc, "changed": bool((before != flat).any())}, out)
    else:
        torch.save({"flat": flat.clone(), "changed": bool((before != flat).any())}, out + ".1")
    dist.destroy_process_group()


def test_real_model_broadcast_and_bucketed_allreduce(tmp_path):
    world, out = 2, str(tmp_path / "real.pt")
    mp.spawn(_worker_real, args=(world, 29535, out), nprocs=world, join=True)
    r0, r1 = torch.load(out), torch.load(out + ".1")
    assert torch.equal(r0["flat"], r1["flat"]) and not r0["changed"] and r1["changed"]  # rank 1 took rank 0's parameters
    assert r0["n_async"] == 4 and r0["n_acc"] == 0 and r0["scale"] == 0.5
    n = r0["g"].numel()
    assert torch.equal(r0["g"], torch.arange(n, dtype=torch.float32) % 97 * 3)  # every element summed over both ranks exactly once


def test_bench_gpus2_self_launches_its_ranks():
    """`python3 bench.py --gpus 2` typed as is (no torchrun, WORLD_SIZE unset): the script must start its two ranks as child processes of
    torch.distributed.run instead of exiting 1 at argument handling.  FALNET_BENCH_DRYRUN=1 stops each rank after the
    rendezvous and one gloo collective, before any GPU call, so this runs on the CPU box; the GPU form is tests/test_gpu_step.py:
    test_bench_two_ranks_reports_allreduce[self]."""
    import json
    import subprocess
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(FALNET_DIST_BACKEND="gloo", FALNET_BENCH_DRYRUN="1")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    last = r.stdout.strip().splitlines()[-1]
    d = json.loads(last)  # the JSON line is the LAST line of stdout
    assert d["dry_run"] is True and d["n_gpus"] == 2 and d["ranks_seen"] == 2


def test_bench_gpus_mismatch_is_refused():
    """WORLD_SIZE set by a launcher but different from --gpus: refused with a message (not silently benchmarked at another size)."""
    import subprocess
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", FALNET_BENCH_DRYRUN="1")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr


def test_bench_launch_table_needs_full():
    """The per-launch table comes from the instrumented pass, a leg of --full: asked for without it, bench.py refuses before any GPU call."""
    import subprocess
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--launch-table", os.devnull], capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "--full" in r.stderr


def test_bench_dump_outputs_budget_and_fixed_sample(tmp_path):
    """bench.dump_outputs on host tensors shaped like a step's result: every array as float32 .npy, 64 MB at most in all (the two flat
    buffers alone are 96 MB here), a large array as the same seeded sample of its elements in every run."""
    import subprocess
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    prog = """
import sys, torch
sys.path.insert(0, sys.argv[1])
import bench
class M:
    def flat_parameters(self):
        return torch.arange(12000000, dtype=torch.float32)
    def flat_gradients(self):
        return -torch.arange(12000000, dtype=torch.float32)
out = {"loss": torch.tensor(1.5), "sm": 0, "ldisp": torch.rand(8, 1, 256, 512, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16),
       "scaler": None}
bench.dump_outputs(sys.argv[2], out, M())
"""
    dumps = []
    for i in range(2):
        d = tmp_path / f"d{i}"
        r = subprocess.run([sys.executable, "-c", prog, root, str(d)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        assert sorted(f.name for f in d.iterdir()) == ["gradients.npy", "ldisp.npy", "loss.npy", "parameters.npy", "sm.npy"]
        assert sum(f.stat().st_size for f in d.iterdir()) <= 64e6
        dumps.append({f.name: np.load(f) for f in d.iterdir()})
    a, b = dumps
    assert all(v.dtype == np.float32 for v in a.values())
    assert float(a["loss.npy"]) == 1.5 and float(a["sm.npy"]) == 0.0
    p = a["parameters.npy"]
    assert p.ndim == 1 and 1000 < p.size < 12000000 and np.all(np.diff(p) > 0)  # sorted indices, no repeats: p holds the indices themselves (exact in f32 below 2**24)
    assert np.array_equal(a["gradients.npy"], -p)  # the same elements of both flat buffers
    for k in a:
        assert np.array_equal(a[k], b[k]), k
