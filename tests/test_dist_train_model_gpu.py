"""train_model.main in its distributed mode, end to end: two ranks sharing ONE MI355X (--dist-backend gloo, LOCAL_RANK 0 on
both), synthetic data, plain and with --num-hierarchical-sequences.  Only rank 0 prints and writes; the checkpoint has the
single-GPU layout (S or K table rows) and loads into a one-GPU model and optimizer and into eval_model; the dev lower bound
counts every dev segment once (it equals the one-process bound of the checkpointed model on the same batches); --continue-from
resumes in distributed mode.  K = 1 over two ranks leaves rank 1 an empty table shard."""
import contextlib
import glob
import io
import os
import re

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

T, F, H, D, S = 20, 16, 32, 16, 9
COMMON = ["--seg-len", str(T), "--mels", str(F), "--z1-hus", str(H), str(H), "--z2-hus", str(H), str(H), "--x-hus", str(H), str(H),
          "--z1-dim", str(D), "--z2-dim", str(D), "--num-seqs", str(S), "--train-segments", "101", "--dev-segments", "37",
          "--training-batch-size", "16", "--dev-batch-size", "16", "--dist-backend", "gloo", "--check-interval", "2", "--seed", "4"]


def _zero_draw(self, eps, B, device):
    """Zero reparameterisation noise everywhere (train and dev): the dev bound becomes a deterministic function of the weights."""
    if eps is not None:
        return eps[0].to(device), eps[1].to(device)
    return torch.zeros(B, self.z2_dim, device=device), torch.zeros(B, self.z1_dim, device=device)


def _worker(rank, world, port, argv_list, ret):
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "pytorch-scalablefhvae_amd")]
    os.environ.update(MASTER_ADDR="127.0.0.1", RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import fhvae_core
    import train_model

    fhvae_core.FHVAEBase._draw = _zero_draw
    outs = []
    for i, argv in enumerate(argv_list):  # (one process group per main() call: main creates and destroys it)
        os.environ["MASTER_PORT"] = str(port + i)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            rc = train_model.main(argv)
        outs.append((rc, buf.getvalue()))
    ret[rank] = outs


def _run(argv_list, tag):
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(2, 28800 + (os.getpid() % 100) * 5 + 500 * tag, argv_list, ret), nprocs=2, join=True)
    return ret[0], ret[1]


def _dev_bounds(text):
    return [float(v) for v in re.findall(r"Validation set lower bound: (-?[0-9.]+)", text)]


def _one_process_dev_bound(model, hs):
    from datasets import SyntheticSegmentPool
    from hierarchical import estimate_pool_mu2
    from train_model import synthetic_split

    x, idx, ns = synthetic_split(37, T, F, S, 4 + 2)
    x = x.cuda()
    with torch.no_grad():
        if hs:
            pool = SyntheticSegmentPool(x, idx, ns, S, torch.device("cuda"))
            mu2 = estimate_pool_mu2(model, pool)
            lbs = [model(f, i, S, n, mu2_table=mu2)[0] for i, f, n in pool.epoch(16, shuffle=False)]
        else:
            lbs = [model(x[s:s + 16], idx[s:s + 16], S, ns[s:s + 16])[0] for s in range(0, 37, 16)]
    return torch.cat(lbs).mean().item()


@pytest.mark.parametrize("hs", [None, 5, 1])
def test_train_model_two_ranks(tmp_path, monkeypatch, hs):
    import eval_model
    import fhvae_core
    import utils
    from hip_optim import FusedAdam

    monkeypatch.setattr(fhvae_core.FHVAEBase, "_draw", _zero_draw)
    exp = str(tmp_path / "exp")
    extra = ["--num-hierarchical-sequences", str(hs)] if hs else []
    first = COMMON + extra + ["--epochs", "2", "--exp-dir", exp]
    resume = COMMON + extra + ["--epochs", "3", "--exp-dir", exp, "--continue-from", os.path.join(exp, "fhvae_run_e1.tar")]
    (r0a, r0b), (r1a, r1b) = _run([first, resume], {None: 0, 5: 1, 1: 2}[hs])
    assert r0a[0] == 0 and r1a[0] == 0 and r0b[0] == 0 and r1b[0] == 0, (r0a, r1a)
    assert r1a[1] == "" and r1b[1] == ""  # only rank 0 prints
    out = r0a[1]
    assert out.count("====> Train set average loss") == 2 and "segments/s" in out
    if not hs:
        # 101 segments in batches of 16: the last batch of 5 is cut to 4 (one segment skipped per epoch)
        assert out.count("dist: 1 segments of the last ragged batch skipped") == 2
    else:
        assert "merge" in out and "hs block" in out
    assert "resumed from" in r0b[1] and "starting at epoch 2" in r0b[1]
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(exp, "*")) if "best_model" not in p)
    assert names == ["args.pkl", "fhvae_run_e0.tar", "fhvae_run_e1.tar", "fhvae_run_e2.tar"]
    ck_path = os.path.join(exp, "fhvae_run_e1.tar")
    ck = torch.load(ck_path, map_location="cpu", weights_only=False)
    rows = hs if hs else S
    assert ck["state_dict"]["mu2_table"].shape == (rows, D) and ck.get("hierarchical_sequences") == hs
    # the single-GPU layout: one model + one FusedAdam load it (one step count for every parameter, table included)
    model, _, optim_state, start, _, _ = utils.load_checkpoint_file(ck_path, False)
    assert start == 2
    model = model.cuda()
    opt = FusedAdam(model.parameters(), lr=1e-3, betas=(0.95, 0.999))
    opt.load_state_dict(optim_state)
    steps = {float(st["step"]) for st in optim_state["state"].values()}
    assert len(steps) == 1 and steps.pop() == float(opt.step_dev.item()) > 0
    # the dev bound the two ranks printed for epoch 1 = the one-process bound of that checkpoint on the same dev batches
    want = _one_process_dev_bound(model.eval(), bool(hs))
    got = _dev_bounds(out)[1]
    assert abs(got - want) <= 1e-4 * abs(want) + 1e-4, (got, want)
    assert abs(ck["values"]["val_lower_bound"] - want) <= 1e-5 * abs(want), (ck["values"], want)
    # eval_model reads it
    assert eval_model.main(["--checkpoint", ck_path, "--out", str(tmp_path / "eval"), "--seg-len", str(T), "--mels", str(F),
                            "--num-seqs", str(S), "--segments", "37", "--seed", "4"]) == 0
    # the distributed resume continued from it and trained on
    ck2 = torch.load(os.path.join(exp, "fhvae_run_e2.tar"), map_location="cpu", weights_only=False)
    assert ck2["epoch"] == 2 and float(ck2["optimizer"]["state"][0]["step"]) > float(ck["optimizer"]["state"][0]["step"])


def _worker_empty_shard(rank, world, port, ret):
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "pytorch-scalablefhvae_amd")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dist_shard import DistributedFHVAE
    from fhvae import FHVAE

    torch.manual_seed(2)
    m = FHVAE(T * F, [H, H], [H, H], D, D, [H, H], seg_len=T, num_seqs=1, reference_compat=False).cuda()
    runner = DistributedFHVAE(m, lr=1e-3, betas=(0.95, 0.999))
    g = torch.Generator().manual_seed(rank)
    for _ in range(2):
        runner.train_step(torch.randn(4, T, F, generator=g).cuda(), torch.zeros(4, dtype=torch.int64).cuda(),
                          torch.randint(20, 200, (4,), generator=g).cuda())
    sd = runner.state_dict()
    cpu = lambda d: {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in d.items()}  # noqa: E731
    opt = dict(sd["optimizer"], state={i: cpu(st) for i, st in sd["optimizer"]["state"].items()})
    ret[rank] = dict(rows=(runner.sh.row0, runner.sh.row1), opt=opt, sd=cpu(sd["state_dict"]))
    dist.destroy_process_group()


def test_empty_shard_checkpoint_step_comes_from_the_nets():
    """K = 1 over two ranks: rank 1's table shard is empty and its table optimizer never steps; the state every rank writes
    carries the nets' step for the table, so either rank's checkpoint loads into one GPU's FusedAdam."""
    from fhvae import FHVAE
    from hip_optim import FusedAdam

    ret = mp.Manager().dict()
    mp.spawn(_worker_empty_shard, args=(2, 29400 + os.getpid() % 150, ret), nprocs=2, join=True)
    assert ret[0]["rows"] == (0, 1) and ret[1]["rows"] == (1, 1)
    for r in range(2):
        st = ret[r]["opt"]["state"]
        assert {float(v["step"]) for v in st.values()} == {2.0}
        m = FHVAE(T * F, [H, H], [H, H], D, D, [H, H], seg_len=T, num_seqs=1, reference_compat=False).cuda()
        m.load_state_dict(ret[r]["sd"])
        opt = FusedAdam(m.parameters(), lr=1e-3, betas=(0.95, 0.999))
        opt.load_state_dict(ret[r]["opt"])
        assert int(opt.step_dev.item()) == 2
