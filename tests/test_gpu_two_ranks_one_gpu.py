"""N > 1 on the hardware that exists here: two ranks share the ONE MI355X of the box and run the REAL kernels, collectives
through gloo (RCCL refuses two ranks on one device).  Everything of the multi-GPU path except RCCL / xGMI itself is then
exercised on the device: per-rank ray shards, pxo_train_fwd_bwd_bucketed's `grads0_ready` event handed to each rank's side
stream, the two-bucket exchange of dist.GradReducer, Adam on the reduced gradient, and -- as a second test -- bench.py's own
multi-rank flow with the sharded extraction records.

Checked: replicas stay BIT-identical over 4 steps (same reduced gradient, same deterministic Adam); 2 x B/2 rays equals the
single-process step on B rays with the same injected randoms (lax.pmean = mean of per-shard means, nerf_sh/train.py:117-118)
to float32 round-off of the gradient sums."""
import json
import os
import socket
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

pytestmark = pytest.mark.gpu
B_GLOBAL, STEPS, N_SP = 1024, 4, 1000


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _problem():
    from oracle import nerf_oracle as O
    from _helpers import make_params, make_rays
    cfg = O.Cfg(sparsity_npoints=N_SP, weight_decay_mult=0.01)
    flat = make_params(cfg)
    rays = make_rays(B_GLOBAL)
    g = torch.Generator().manual_seed(77)
    px = torch.rand(B_GLOBAL, 3, generator=g)
    rnd = [(torch.rand(B_GLOBAL, 64, generator=g), torch.rand(B_GLOBAL, 128, generator=g),
            (torch.rand(N_SP, 3, generator=g) * 2 - 1) * 1.5) for _ in range(STEPS)]
    return cfg, flat, rays, px, rnd


def _run(rank, world, comm, dev, skip=0):
    from _helpers import pxo_cfg
    from plenoctree_amd import dist, ops
    from plenoctree_amd.nerf_sh.nerf import models, utils
    cfg, flat, rays, px, rnd = _problem()
    pcfg = pxo_cfg(ops, cfg)
    pcfg.skip_zero_rows = skip
    model = models.NerfModel(pcfg)
    state = models.TrainState(pcfg, flat.clone().to(dev))
    reducer = dist.GradReducer(comm, dev) if world > 1 else None
    per = B_GLOBAL // world
    sl = slice(rank * per, (rank + 1) * per)
    for step in range(STEPS):
        t_rand, u, sp = rnd[step]
        batch = {"rays": utils.Rays(*[r[sl].contiguous().to(dev) for r in rays]), "pixels": px[sl].contiguous().to(dev)}
        models.train_step(model, state, batch, 5e-4, t_rand=t_rand[sl].contiguous().to(dev), u=u[sl].contiguous().to(dev),
                          sp_points=sp.to(dev), world_size=world, reducer=reducer)
    torch.cuda.synchronize()
    return state.params.cpu(), state.stats.cpu(), state.grads.cpu() * (1.0 / world)


def _worker(rank, world, port, outdir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from plenoctree_amd import dist
    torch.cuda.set_device(0)
    comm = dist.init_from_env(backend="gloo")
    assert comm.world == world
    params, stats, grads = _run(rank, world, comm, torch.device("cuda", 0))
    p1, s1, g1 = _run(rank, world, comm, torch.device("cuda", 0), skip=1)      # the CLI's default reverse pass
    torch.save({"params": params, "stats": stats, "grads": grads, "params_skip": p1, "stats_skip": s1, "grads_skip": g1},
               os.path.join(outdir, f"rank{rank}.pt"))
    comm.barrier()
    comm.shutdown()


@pytest.mark.timeout(900)
def test_two_ranks_on_one_gpu_match_the_single_process_step():
    from plenoctree_amd import dist
    world = 2
    with tempfile.TemporaryDirectory() as outdir:
        mp.spawn(_worker, args=(world, _free_port(), outdir), nprocs=world, join=True)
        res = [torch.load(os.path.join(outdir, f"rank{r}.pt")) for r in range(world)]
    assert torch.equal(res[0]["params"], res[1]["params"]) and torch.equal(res[0]["stats"], res[1]["stats"])
    assert torch.equal(res[0]["grads"], res[1]["grads"])
    # ... and the zero-row skipping reverse pass (each rank with its own live flags) leaves every bit where it was
    for r in res:
        assert torch.equal(r["params_skip"], r["params"]) and torch.equal(r["stats_skip"], r["stats"])
        assert torch.equal(r["grads_skip"], r["grads"])
    single_p, single_s, single_g = _run(0, 1, dist.Comm(), torch.device("cuda", 0))
    # last step's gradient: mean over the two shards' gradients vs the full-batch gradient.  The ray terms are means over B
    # rays either way; the sparsity and weight-decay terms are identical on both ranks (same points, same parameters)
    g2, g1 = res[0]["grads"].double(), single_g.double()
    rel = float((g2 - g1).norm() / g1.norm())
    print(f"2 ranks x {B_GLOBAL // 2} rays vs 1 x {B_GLOBAL}: last-step gradient rel L2 {rel:.2e}")
    assert rel < 2e-3, rel                       # parameters of the two runs drifted apart by 3 Adam steps of round-off before it
    diff = (res[0]["params"] - single_p).abs()
    assert float(diff.max()) < 2.5e-3 and float(diff.mean()) < 2e-5, (float(diff.max()), float(diff.mean()))
    np.testing.assert_allclose(res[0]["stats"][0].item(), single_s[0].item(), rtol=2e-3)


@pytest.mark.timeout(900)
def test_bench_two_ranks_sharing_the_gpu():
    """bench.py --gpus 2 --backend gloo --share-gpu, launched the way the driver launches N > 1 (torch.distributed.run): the
    real kernels under the real multi-rank control flow -- 2 collectives per step, strong512 inside the existing group, x-slab
    sharded 64^3 grid + all-gather, camera-sharded weight mask + max-all-reduce, sharded eval render -- one JSON line."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--share-gpu", "--full",
           "--steps", "4", "--warmup", "1", "--batch", "1024", "--grid-reso", "64", "--eval-step", "6", "--converge-steps", "30",
           "--converge-views", "1", "--image-factor", "8", "--no-cpu-baseline", "--extras", "converge,strong512,render_fwd,grid512"]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=800)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["nccl_ranks_seen"] == 2 and out["collectives_per_step"] == 2
    assert out["config"]["global_batch"] == 2048 and np.isfinite(out["final_stats"]["loss"])
    assert out["strong512"]["collectives_per_step"] == 2 and "rccl_init_error" not in out["strong512"]
    g = out["grid512"]
    assert g["points"] == 64 ** 3 and "2 GPU(s)" in g["sharding"] and g["tree_nodes"] >= 1
    assert 5.0 < out["eval_psnr"] < 60.0 and out["converge"]["view_size"] == [100, 100]
    assert "sharing ONE GPU" in out["dry_run"]
