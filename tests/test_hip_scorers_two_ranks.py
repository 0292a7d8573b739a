"""GPU, two processes sharing the one MI355X (the tests/test_hip_two_ranks.py pattern: gloo collectives carrying device
tensors): StandardRec with the MLP scorer (cfg.scoring 'fc') -- the data-parallel grad step, rec_model.* included, against
the single-process step over the whole batch, and the rank-sharded evaluation epoch (the scorer's news-side projection over
the all-gathered table) against the single-process epoch."""
import os
import socket
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu

C = dict(model="standard", E=32, bias=True, h=4, D=32, H=8, S=6)
N_SESS, SEED = 48, 5


class Cfg(dict):
    __getattr__ = dict.__getitem__


def _world():
    from xnrs_amd import synth
    return synth.click_world(n_news=120, n_sess=64)


def _model(dev):
    from xnrs_amd import synth
    from xnrs_amd.models import make_model
    torch.manual_seed(0)
    return make_model(Cfg(dict(synth.model_cfg(C), scoring="fc"))).to(dev).eval()


def _batch(dev, lo, hi):
    from xnrs_amd.data import DeviceBatcher
    store, beh = _world()
    store, beh = store.to(dev), beh.to(dev)
    sess = torch.arange(N_SESS, device=dev)
    hist, cand, targets = DeviceBatcher(beh, l_hist=8).train_batch(sess, n_neg=4, seed=SEED)
    labels = beh.theme_labels[sess]
    return store, hist[lo:hi], cand[lo:hi], targets[lo:hi], labels[lo:hi]


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank(rank, world, port, path):
    import torch.distributed as dist

    from xnrs_amd import distributed as D
    from xnrs_amd.losses import contrastive_loss
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda", 0)
    lo, hi = D.shard_range(N_SESS, rank, world)
    store, hist, cand, targets, labels = _batch(dev, lo, hi)
    model = _model(dev)
    D.broadcast_parameters(model)
    layout = D.ShardLayout.uniform(hi - lo)
    bucket = D.GradBucket(model.parameters())
    bucket.zero_grad()
    r, u, _ = model.forward_ids(store.x, store.m, hist, cand, return_embeddings=True)
    rec = torch.nn.functional.mse_loss(torch.relu(r), targets)
    ue, lab = D.gather_embeddings_and_labels(u.squeeze(1), labels, layout)
    loss = D.global_train_loss(rec, hi - lo, N_SESS, contrastive_loss(ue, lab, 0.08), 0.1)
    loss.backward()
    bucket.allreduce()
    if rank == 0:
        torch.save({k: p.grad.detach().cpu() for k, p in model.named_parameters() if p.grad is not None}, path)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_with_the_mlp_scorer_equal_the_single_process_step():
    import torch.multiprocessing as mp

    from xnrs_amd.losses import contrastive_loss
    dev = torch.device("cuda", 0)
    store, hist, cand, targets, labels = _batch(dev, 0, N_SESS)
    model = _model(dev)
    r, u, _ = model.forward_ids(store.x, store.m, hist, cand, return_embeddings=True)
    loss = torch.nn.functional.mse_loss(torch.relu(r), targets) + 0.1 * contrastive_loss(u.squeeze(1), labels, 0.08)
    loss.backward()
    ref = {k: p.grad.detach().cpu() for k, p in model.named_parameters() if p.grad is not None}
    assert {"rec_model.fc1.weight", "rec_model.fc1.bias", "rec_model.fc2.weight", "rec_model.fc2.bias"} <= set(ref)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "rank0.pt")
        mp.spawn(_rank, args=(2, _port(), path), nprocs=2, join=True)
        got = torch.load(path, weights_only=True)
    assert set(ref) <= set(got)
    for k in set(got) - set(ref):
        assert not got[k].any(), k
    gmax = max(v.abs().max().item() for v in ref.values())
    for k, g in ref.items():
        scale = max(g.abs().max().item(), 1e-3 * gmax)
        assert (got[k] - g).abs().max().item() / scale <= 1e-4, k


def _eval_rank(rank, world, port, path):
    import torch.distributed as dist

    from xnrs_amd import distributed as D
    from xnrs_amd.evaluation import evaluate
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda", 0)
    store, beh = _world()
    model = _model(dev)
    D.broadcast_parameters(model)
    torch.save(evaluate(model, store.to(dev), beh.to(dev), l_hist=8, batch=16), f"{path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_rank_sharded_evaluation_with_the_mlp_scorer_equals_the_single_process_epoch():
    import torch.multiprocessing as mp

    from xnrs_amd.evaluation import evaluate
    dev = torch.device("cuda", 0)
    store, beh = _world()
    ref = evaluate(_model(dev), store.to(dev), beh.to(dev), l_hist=8, batch=16, distributed=False)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "res")
        mp.spawn(_eval_rank, args=(2, _port(), path), nprocs=2, join=True)
        got = [torch.load(f"{path}.{r}", weights_only=True) for r in range(2)]
    for res in got:
        for k in ref:
            assert abs(res[k] - ref[k]) <= 1e-6 * max(1.0, abs(ref[k])), (k, res[k], ref[k])
