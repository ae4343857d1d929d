"""MI355X: data-parallel training ("Training").  Two ranks share the one GPU with the collectives over gloo
(CH_DIST_BACKEND=gloo) -- a rehearsal of the one-process-per-GPU layout, not a scaling run -- and one rank drives real RCCL.  Every
rank is a fresh child process under its own `timeout`; the first child that fails ends the test (the others are killed, nothing is
retried)."""
import json
import os
import socket
import subprocess
import sys
from concurrent.futures import FIRST_COMPLETED, ThreadPoolExecutor, wait

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

WORKER = os.path.join(ROOT, "tests", "train_ddp_worker.py")
MODEL = ["model.backbone.name=synthetic/clip-vit-small-patch16", "model.nbit=64"]
SETUP = ["exp=hashing", "optim=sgd", "scheduler=no_decay", "batch_size=16", "dataset=synthetic_cub200", "dataset.limit=64", "dataset.nclass=8"]
CHILD_LIMIT = 300       # seconds, per child process


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_env(env, rank, world, port, backend="gloo"):
    return dict(env, WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                CH_DIST_BACKEND=backend)


def _run_children(jobs, cwd):
    """jobs: [(name, argv, env)] started together, each under its own `timeout`.  Returns when all have ended with status 0; the first
    one that ends otherwise fails the test at once and the rest are killed."""
    procs = {}
    for name, argv, env in jobs:
        log = open(os.path.join(cwd, f"{name}.log"), "w")
        procs[name] = (subprocess.Popen(["timeout", "-k", "10", str(CHILD_LIMIT)] + argv, env=env, cwd=cwd, stdout=log,
                                        stderr=subprocess.STDOUT), log)
    with ThreadPoolExecutor(len(procs)) as pool:
        pending = {pool.submit(p.wait): name for name, (p, _) in procs.items()}
        try:
            while pending:
                done, _ = wait(list(pending), return_when=FIRST_COMPLETED)
                for f in done:
                    name = pending.pop(f)
                    if f.result() != 0:
                        tail = open(os.path.join(cwd, f"{name}.log")).read()[-4000:]
                        pytest.fail(f"child {name} ended with status {f.result()}:\n{tail}")
        finally:
            for p, log in procs.values():
                if p.poll() is None:
                    p.kill()
                log.close()


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _arenas(state):
    """the buffers of one run grouped as the step all-reduces them: adapter arena, backbone arena, the torch-side parameters as one vector"""
    out = {k[len("arena/"):]: v for k, v in state.items() if k.startswith("arena/")}
    out["torch_side"] = torch.cat([v.reshape(-1) for k, v in sorted(state.items()) if k.startswith("torch/")])
    return out


def _update_size(moved):
    """relative L2 of the three steps' own update (final - start, over start) per arena of `_arenas`, from the single-process run"""
    groups = {}
    for g, final, start in moved.values():
        d, n = groups.get(g, (0.0, 0.0))
        groups[g] = (d + float((final.double() - start.double()).pow(2).sum()), n + float(start.double().pow(2).sum()))
    return {g: (d / n) ** 0.5 for g, (d, n) in groups.items()}


@pytest.mark.parametrize("backbone_lr_scale", [0, 0.1], ids=["frozen", "trainable"])
def test_two_ranks_of_8_take_the_steps_of_one_process_at_batch_16(tmp_path, backbone_lr_scale):
    """Three SGD steps in one process at batch 16 against the same three steps as 2 ranks of 8.
    Exact: (a) after every step both ranks hold bit-identical parameter arenas, torch-side parameters and batch-norm running statistics
    (asserted in the children through an all_gather of a 64-bit checksum per buffer, and again here on the saved final state); (b) the
    dataset indices of rank 0's and rank 1's step-i batches, concatenated, are the single-process step-i batch.
    Measured: relative L2 per arena between the 2-rank and the single-process parameters after step 3, against the yardstick of the
    single-process run repeated with every batch's rows reversed (the same sums in another fp32 order; no code of the data-parallel path).
    Asserted: yardstick > 0 and 2-rank difference <= 4 x yardstick, per arena.

    Sensitivity, measured and asserted in the test itself: the relative L2 of the three steps' own update (single process, final against
    start) per arena must be at least 2 x the bound; on MI355X it is 23 x to 48 x the bound (update 1.2e-3 .. 3.5e-2).
    A fault that rescales or drops a gradient moves the parameters by a multiple of that update.  The loss not scaled by 1 / world_size
    doubles every gradient, so the difference to one process is the whole update: caught by the bound, which is its only guard here (both
    ranks would apply the same doubled gradient).  An all-reduce of one of the three buffers left out leaves each rank with the gradient of
    its own 8 images: the ranks part at step 1, caught by (a), the children's checksum exchange.  `hash_bn` on per-rank statistics gives the
    ranks different running statistics: caught by (a) as well, which covers those buffers."""
    cwd = str(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    lr = "optim.lr=0.02"
    args = SETUP + MODEL + [lr, f"backbone_lr_scale={backbone_lr_scale}", "data_dir=" + cwd]
    port = _free_port()
    jobs = [("single", [sys.executable, WORKER, os.path.join(cwd, "single.pt"), "single", "3"] + args + ["logdir=" + cwd + "/run_single"], env),
            ("reversed", [sys.executable, WORKER, os.path.join(cwd, "reversed.pt"), "reversed", "3"] + args + ["logdir=" + cwd + "/run_rev"], env)]
    for r in range(2):
        jobs.append((f"rank{r}", [sys.executable, WORKER, os.path.join(cwd, f"rank{r}.pt"), "ranks", "3"] + args
                     + ["logdir=" + cwd + "/run_ranks"], _rank_env(env, r, 2, port)))
    _run_children(jobs, cwd)
    single, rev, r0, r1 = (torch.load(os.path.join(cwd, f"{n}.pt")) for n in ("single", "reversed", "rank0", "rank1"))
    # (b) the same images, step by step
    assert len(single["indices"]) == len(r0["indices"]) == len(r1["indices"]) == 3
    for i in range(3):
        assert r0["indices"][i].numel() == r1["indices"][i].numel() == 8
        assert torch.equal(torch.cat([r0["indices"][i], r1["indices"][i]]), single["indices"][i]), i
        assert torch.equal(rev["indices"][i], single["indices"][i].flip(0))
    # (a) bit-identical ranks
    assert set(r0["state"]) == set(r1["state"]) == set(single["state"])
    for k in r0["state"]:
        assert torch.equal(r0["state"][k], r1["state"][k]), k
    assert ("arena/backbone" in r0["state"]) == (backbone_lr_scale != 0)
    assert r0["fused_steps"] == single["fused_steps"] == 3
    # measured: rounding-order noise of the same sums
    a1, ar, a2 = _arenas(single["state"]), _arenas(rev["state"]), _arenas(r0["state"])
    for name in a1:
        yard, diff = _rel_l2(ar[name], a1[name]), _rel_l2(a2[name], a1[name])
        print(f"backbone_lr_scale={backbone_lr_scale} {name}: 2 ranks vs 1 process {diff:.3e}; rows reversed vs 1 process (yardstick) {yard:.3e}")
    for name in a1:
        yard, diff = _rel_l2(ar[name], a1[name]), _rel_l2(a2[name], a1[name])
        assert yard > 0, name
        assert diff <= 4 * yard, (name, diff, yard)
    # sensitivity: a lost 1 / world_size doubles every gradient, so (SGD is linear in the gradients up to weight decay) it doubles the
    # update and the difference to the single-process run IS the update; the bound can only catch that where the update is well above it
    upd = _update_size(single["moved"])
    for name in a1:
        yard = _rel_l2(ar[name], a1[name])
        print(f"backbone_lr_scale={backbone_lr_scale} {name}: update of 3 steps {upd[name]:.3e} = {upd[name] / (4 * yard):.1f} x the bound")
        assert upd[name] >= 2 * 4 * yard, (name, upd[name], yard)
    print(f"losses: single {single['loss']:.6f} reversed {rev['loss']:.6f} rank0 {r0['loss']:.6f} rank1 {r1['loss']:.6f}")


def test_main_v2_trains_as_two_ranks(tmp_path):
    """`main_v2.py exp=hashing epochs=2 eval_interval=2 batch_size=16 backbone_lr_scale=0.1` as 2 ranks: each step's record says
    world_size 2 / 8 images per rank, the loss falls, ONE models/last.pth exists and loads, and the single-process `--config-name val.yaml`
    run on that run directory reproduces the mAP the training run recorded."""
    cwd = str(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    logdir = os.path.join(cwd, "run")
    common = ["dataset=synthetic_cub200", "dataset.limit=64", "dataset.nclass=8", "data_dir=" + cwd]
    argv = [sys.executable, os.path.join(ROOT, "main_v2.py"), "exp=hashing", "optim=sgd", "optim.lr=0.02", "scheduler=no_decay", "epochs=2",
            "eval_interval=2", "batch_size=16", "backbone_lr_scale=0.1", "logdir=" + logdir] + MODEL + common
    port = _free_port()
    _run_children([(f"rank{r}", argv, _rank_env(env, r, 2, port)) for r in range(2)], cwd)
    tr = json.load(open(os.path.join(logdir, "train_history.json")))
    te = json.load(open(os.path.join(logdir, "test_history.json")))
    assert len(tr) == 2 and all(t["world_size"] == 2 and t["images_per_rank"] == 8 for t in tr)
    print("train losses", [t["train_loss"] for t in tr])
    assert tr[-1]["train_loss"] < tr[0]["train_loss"]
    found = [os.path.join(d, f) for d, _, fs in os.walk(cwd) for f in fs if f == "last.pth" and os.path.basename(d) == "models"]
    assert found == [os.path.join(logdir, "models", "last.pth")], found
    ck = torch.load(found[0], map_location="cpu")
    assert "hash_fc.weight" in ck and all(torch.isfinite(v).all() for v in ck.values() if torch.is_tensor(v) and v.is_floating_point())
    assert not [f for f in os.listdir(logdir) if f.endswith(".tmp")]
    ev = os.path.join(cwd, "ev")
    _run_children([("val", [sys.executable, os.path.join(ROOT, "main_v2.py"), "--config-name", "val.yaml", "logdir=" + logdir, "batch_size=32",
                            "eval_logdir=" + ev] + common, env)], cwd)
    hist = json.load(open(os.path.join(ev, "history.json")))
    assert len(te) == 1 and abs(hist["mAP"] - te[0]["mAP"]) < 1e-12, (hist["mAP"], te[0]["mAP"])


def test_rccl_runs_the_collectives_of_a_training_step(tmp_path):
    """Real RCCL (backend "nccl"), one rank, CH_FORCE_COLLECTIVES=1: one training step with a trainable backbone whose gradient all-reduces
    (adapter arena, backbone arena, flat torch-side buffer), batch-norm all-reduces (forward and backward), key agreement and start-up
    broadcast run as collectives on GPU tensors.  In a one-rank group they are identities: the parameters afterwards are bit-equal to the
    same step with the collectives skipped."""
    cwd = str(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0", CH_DIST_BACKEND="nccl", MASTER_ADDR="127.0.0.1")
    env.pop("CH_FORCE_COLLECTIVES", None)
    args = SETUP + MODEL + ["optim.lr=0.02", "backbone_lr_scale=0.1", "data_dir=" + cwd]
    jobs = []
    for name, extra in (("forced", {"CH_FORCE_COLLECTIVES": "1"}), ("skipped", {})):
        jobs.append((name, [sys.executable, WORKER, os.path.join(cwd, f"{name}.pt"), "solo", "1"] + args + [f"logdir={cwd}/run_{name}"],
                     dict(env, MASTER_PORT=str(_free_port()), **extra)))
    _run_children(jobs, cwd)
    forced, skipped = torch.load(os.path.join(cwd, "forced.pt")), torch.load(os.path.join(cwd, "skipped.pt"))
    # batch-norm forward + backward, three gradient buffers, the key agreement
    assert forced["all_reduce_calls"] == 6 and skipped["all_reduce_calls"] == 0, (forced["all_reduce_calls"], skipped["all_reduce_calls"])
    assert set(forced["state"]) == set(skipped["state"]) and "arena/backbone" in forced["state"]
    for k in forced["state"]:
        assert torch.equal(forced["state"][k], skipped["state"][k]), k
    assert forced["fused_steps"] == 1
