#!/usr/bin/env python
"""End-to-end example in the shape of the reference's train.py / ContrastiveRankingTrainer (training.py:402-431),
entirely on the device: resident news table -> device batch assembly -> forward_ids (id gather fused into the first
GEMM) -> relu/MSE + lambda * fused InfoNCE -> hand-written HIP backward -> Adam -> device evaluation.

    python examples/train_synthetic.py [--model NRMS|standard] [--steps 300] [--batch 64] [--bf16x3]
                                      [--full-table-loss | --mined-negatives M [--negatives-temperature T]] [--distill]

--full-table-loss (off by default) trains with losses.full_table_loss instead: every clicked news of a session against ALL
news of the table encoded in that step, the objective evaluate_full_ranking measures.
--mined-negatives M (mutually exclusive with it) trains with losses.mined_negatives_loss: the same clicks against the M news
of that table the session's user scores highest in that step (topk_deep mines them, the listed loss reads their rows in place).
--negatives-temperature T draws the M negatives instead, P(news first) ~ exp(score / T) without replacement (topk_sample, the
step number as the seed): the hardest rows are where the false negatives live.
--distill trains the model with the MLP ('fc') scorer as a teacher on clicks as above, then a dot-product student from the
teacher alone (losses.distillation_loss over the student's own pool of 128), and prints evaluation.list_recall of the
teacher's top 10 inside the student's pool, and hit@10 of both, before and after.

Synthetic click world (xnrs_amd.synth.click_world): news carry a topic direction in their tokens, a user clicks news of
its own topic -- so the ranking metrics have to rise if the whole stack (forward, gradients, optimiser, evaluation) is
right.  Needs an MI355X; there is no CPU fallback."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xnrs_amd import evaluation, hip, synth  # noqa: E402
from xnrs_amd.data import DeviceBatcher  # noqa: E402
from xnrs_amd.losses import contrastive_loss, distillation_loss, full_table_loss, mined_negatives_loss  # noqa: E402
from xnrs_amd.models import make_model  # noqa: E402


class Cfg(dict):
    __getattr__ = dict.__getitem__


def distill(teacher, cfg, store, beh, args, dev):
    """--distill: a dot-product student trained from the frozen teacher's soft targets alone, never from a click"""
    teacher.eval()
    for p in teacher.parameters():
        p.requires_grad_(False)
    teacher_table = evaluation.encode_news_table(teacher, store)  # the teacher is frozen: its table is encoded once
    top10 = evaluation.recommend(teacher, store, beh, args.hist, k=10)[0]
    torch.manual_seed(1)
    student = make_model(Cfg(dict(cfg, scoring="dot"))).to(dev)
    student.news_encoder.skip_empty = True
    opt = torch.optim.Adam(student.parameters(), lr=1e-3)

    def report(tag):
        student.eval()
        pool = evaluation.recommend(student, store, beh, args.hist, k=128)[0]
        recall = evaluation.list_recall(pool, top10).mean().item()
        hit = {n: evaluation.evaluate_full_ranking(m, store, beh, args.hist, ks=(10,))["hit@10"]
               for n, m in (("teacher", teacher), ("student", student))}
        print(f"distill {tag}: the student's pool of 128 holds {recall:.4f} of the teacher's top 10; "
              f"hit@10 teacher {hit['teacher']:.4f}, student {hit['student']:.4f}")
        student.train()
        return recall

    before = report("before")
    for step in range(args.steps):
        sess = torch.randint(0, len(beh), (args.batch,), device=dev)
        opt.zero_grad()
        # (the teacher was regressed on 0 / 1 targets, so its scores over a pool span about one unit: at temperature 1 the
        # targets are nearly uniform and say little; 0.1 stretches them to about ten)
        loss = distillation_loss(student, teacher, store, beh, sess, args.hist, pool=128, temperature=0.1,
                                 teacher_table=teacher_table)
        loss.backward()
        opt.step()
        if step % 50 == 0 or step == args.steps - 1:
            print(f"distill step {step:4d}  KL(teacher || student) {loss.item():.6f}")
    after = report("after ")
    assert after > before, "the student's pool did not move towards the teacher's list"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="NRMS", choices=("NRMS", "standard"))
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--hist", type=int, default=8)
    ap.add_argument("--bf16x3", action="store_true", help="forward GEMMs + dX products on the bf16 matrix cores (fp32-grade)")
    which = ap.add_mutually_exclusive_group()
    which.add_argument("--full-table-loss", action="store_true",
                       help="train with the softmax ranking loss over the whole news table (losses.full_table_loss)")
    which.add_argument("--mined-negatives", type=int, default=0, metavar="M",
                       help="train with the ranking loss over the M hardest negatives of each session, mined per step "
                            "(losses.mined_negatives_loss, 1 <= M <= 1024)")
    ap.add_argument("--negatives-temperature", type=float, default=None, metavar="T",
                    help="with --mined-negatives: draw the M negatives with probability ~ exp(score / T) instead of taking the "
                         "M hardest (losses.mined_negatives_loss(temperature=T, seed=step))")
    ap.add_argument("--distill", action="store_true",
                    help="train the model with the MLP ('fc') scorer as a TEACHER on clicks, then a dot-product student from "
                         "the teacher's soft targets alone (losses.distillation_loss) and print how much of the teacher's "
                         "top 10 the student's pool of 128 holds before and after (evaluation.list_recall)")
    ap.add_argument("--explain", action="store_true",
                    help="after training: recommend() three news for session 0 and explain_recommendations() for them")
    args = ap.parse_args()
    if args.negatives_temperature is not None and not args.mined_negatives:
        ap.error("--negatives-temperature goes with --mined-negatives M")
    dev = "cuda:0"
    if args.bf16x3:
        hip.set_gemm_mode(hip.GEMM_BF16X3)
    torch.manual_seed(0)
    store, beh = synth.click_world(n_news=2000, n_sess=4000, S=12, D=64, n_topics=6)
    store, beh = store.to(dev), beh.to(dev)
    cfg = Cfg(synth.model_cfg(dict(model=args.model, E=64, bias=True, h=4, D=64, H=args.hist, S=12)))
    if args.distill:
        cfg["scoring"] = "fc"  # the teacher: a scorer that costs 64x the dot product per ranked row
    model = make_model(cfg).to(dev)
    model.news_encoder.skip_empty = True          # empty history slots share one encoded representative (exact)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    batcher = DeviceBatcher(beh, l_hist=args.hist)
    model.eval()
    before = evaluation.evaluate(model, store, beh, args.hist, batch=1024)
    print("before:", {k: round(v, 4) for k, v in before.items()})
    model.train()
    t0 = time.perf_counter()
    for step in range(args.steps):
        sess = torch.randint(0, len(beh), (args.batch,), device=dev)
        opt.zero_grad()
        if args.full_table_loss:
            loss = full_table_loss(model, store, beh, sess, args.hist)
        elif args.mined_negatives:
            sampling = {} if args.negatives_temperature is None else dict(temperature=args.negatives_temperature, seed=step)
            loss = mined_negatives_loss(model, store, beh, sess, args.hist, n_negatives=args.mined_negatives, **sampling)
        else:
            hist, cand, targets = batcher.train_batch(sess, n_neg=4, seed=step)
            r, u, _ = model.forward_ids(store.x, store.m, hist, cand, return_embeddings=True)
            # (the MLP scorer of --distill starts with every score below 0, where relu passes no gradient and the loss stays
            # at mean(targets^2) = 0.2000 for good: its teacher is regressed on the raw score)
            loss = torch.nn.functional.mse_loss(r if args.distill else torch.relu(r), targets) + \
                0.1 * contrastive_loss(u.squeeze(1), beh.theme_labels[sess], 0.08)
        loss.backward()
        opt.step()
        if step % 50 == 0 or step == args.steps - 1:
            print(f"step {step:4d}  loss {loss.item():.4f}")
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    model.eval()
    after = evaluation.evaluate(model, store, beh, args.hist, batch=1024)
    print("after: ", {k: round(v, 4) for k, v in after.items()})
    print(f"{args.steps} steps of {args.batch} impressions in {dt:.2f} s = {args.steps * args.batch / dt:.0f} impressions/s (tiny model: launch-bound)")
    assert after["auc"] > before["auc"] + 0.1, "the model did not learn"
    if args.distill:
        distill(model, cfg, store, beh, args, dev)
    if args.explain:
        # what does session 0 get, and which news of its history speak for each of those rows?
        from xnrs_amd.explain import explain_recommendations
        rows, scores = evaluation.recommend(model, store, beh, args.hist, k=3, sessions=[0])
        out = explain_recommendations(model, store, beh, args.hist, 0, rows[0], n_steps=50)
        for j, row in enumerate(rows[0].tolist()):
            print(f"session 0 <- row {row} (score {scores[0, j].item():.3f}): attribution per history news",
                  [round(v, 3) for v in out["news_attribution"][j].tolist()])


if __name__ == "__main__":
    main()
