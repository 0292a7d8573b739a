#!/usr/bin/env python
"""bench.py -- impressions/s (encode + score) of the xnrs hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

One "step" = one pass of the hot path over one batch of synthetic MIND-shaped impressions whose
token tensors are ALREADY RESIDENT in HBM: encode H history + C candidate news per impression with
the NRMS news encoder, one user vector, C dot-product scores (ParentRec._forward,
xnrs/models/components/parent.py:31-34), eval mode, no dedup.  Workload = BASELINE.json configs[2]
at the reference's shipped token shape (config/mind_small_NRMS.yml): B=512, H=50, C=5, S=50, D=768,
16 heads, E=256.  configs[1] (news encoder only, 1024 news) is reported under "extra" (--full).

N>1: one process per GPU (launched by torch.distributed.run), impressions sharded by user, no
data-path collective (weak scaling: every rank owns a full B=512 batch); the barrier/MAX reduction
around the timed region is the only communication.

A plain run sets up, runs W warm-up and K timed steps, writes the scores of the last timed step under
--dump-outputs DIR (the inputs are seeded: the same arguments give the same inputs), and prints one JSON
line (value, ms_per_step = milliseconds per timed step, dtype, config, whole_path).  Everything else is
measured with --full only (--no-cpu-baseline / --no-extra drop parts of it); with --full the JSON line
also carries
  roofline     : the dominant kernel (the fused Q/K/V projection, an fp32-MFMA GEMM) -- algorithmic
                 FLOPs per launch / its average launch duration, measured with HIP events inside
                 the timed region (xnrs_profile_* in include/xnrs_hip.h), against the 157.3 TFLOP/s
                 fp32 matrix peak (MI355X_MICROARCH.md).
  cpu_baseline : the CPU oracle (oracle/xnrs_oracle.py, kind "port": the reference itself cannot
                 travel to the GPU box) timed on the host cores on a bounded sample of the same
                 workload, rank 0 at N=1 only.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

# hipGraph replays (extra.*.hipgraph_replay): ROCm 7.2's graph packet-capture path returned stale data between kernel nodes on
# gfx950 (tools/debug_graph_step.py); read by the runtime when it loads, so set before torch is imported.
# It has no effect on the eager launches that every headline number is measured with.
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from xnrs_amd import hip, synth  # noqa: E402
from xnrs_amd.models import make_model  # noqa: E402

FP32_MFMA_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md, chip-level parameters
BF16_MFMA_PEAK_TFLOPS = 2500.0  # dense, same table
# forward-GEMM arithmetic modes (include/xnrs_hip.h: xnrs_set_gemm_mode): name, bf16 MFMA products per fp32 product
GEMM_MODES = {0: ("f32", 1), 1: ("f32 via bf16x3 split operands (6 bf16 MFMA products, fp32 accumulate)", 6),
              2: ("f32 via bf16x2 split operands (3 bf16 MFMA products, fp32 accumulate)", 3)}
HBM_PEAK_GBS = 8000.0

WORKLOAD = dict(B=512, H=50, C=5, S=50, D=768, h=16, E=256, A=256)


class Cfg(dict):
    __getattr__ = dict.__getitem__


def news_flops(S, D, A, E, att=True, head=True, folded=False):
    """algorithmic FLOPs per news item.  folded=True: what the library EXECUTES in inference when
    the out-projection is folded behind the pooling: the S x D x D out-projection becomes one
    D x D product per news (the A x D x D folded weight is per call, not per news)."""
    f = 2 * S * D * A + 2 * S * A + 2 * S * D
    if att:
        # folded: one D x D product per news -- and none at all behind a head (round 4: W0 . Wo folded into the head's first
        # layer, include/xnrs_hip.h xnrs_head_params.w0_folded)
        per_news = 0 if (head and hip.FOLD_HEAD) else 2 * D * D
        f += (6 * S * D * D + per_news if folded else 8 * S * D * D) + 4 * S * S * D
    if head:
        f += 2 * D * E + 2 * E * E
    return f


def fold_on():
    """Does the library fold the out-projection behind the pooling?  (XNRS_FOLD_OUT=0: no.)"""
    return os.environ.get("XNRS_FOLD_OUT", "1") != "0"


def impression_flops(w, folded=False):
    n = (w["H"] + w["C"]) * news_flops(w["S"], w["D"], w["A"], w["E"], folded=folded)
    proj = (6 * w["H"] + 2) if folded else 8 * w["H"]
    u = proj * w["E"] ** 2 + 4 * w["H"] ** 2 * w["E"] + 2 * w["H"] * w["E"] * w["A"] + 2 * w["H"] * w["A"] + 2 * w["H"] * w["E"]
    return n + u + 2 * w["C"] * w["E"]


def impression_bytes(w):
    per_news = 4 * w["S"] * w["D"] + 4 * w["S"] + 4 * w["E"] + 4
    return (w["H"] + w["C"]) * per_news + 4 * w["C"]


def build_model(w, device, seed=1234, model_name="NRMS"):
    c = dict(model=model_name, E=w["E"], bias=False, h=w["h"], D=w["D"], H=w["H"], S=w["S"])
    model = make_model(Cfg(synth.model_cfg(c)))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = synth.fill_state_dict(shapes, seed)
    model.load_state_dict(sd)
    return model.eval().to(device), sd


def make_inputs(w, device, seed, full_history=False):
    """SURVEY.md section 8d inputs: token length ~ U{5..S}, history length ~ U{1..H} (trailing slots all-zero).
    full_history=True keeps every history slot live (no all-zero news rows: the GEMM then multiplies random data
    everywhere -- the DVFS-honest variant of the same step)."""
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    B, H, C, S, D = w["B"], w["H"], w["C"], w["S"], w["D"]
    hx, hm = synth.device_tokens(gen, B * H, S, D, device)
    # ragged histories: trailing slots of each impression are empty (all-zero x and m, dataset.py:82-85)
    n_hist = torch.randint(1, H + 1, (B, 1), generator=gen, device=device)
    if full_history:
        n_hist = torch.full_like(n_hist, H)
    slot_valid = (torch.arange(H, device=device)[None, :] < n_hist).reshape(B * H, 1, 1).to(torch.float32)
    hx.mul_(slot_valid)
    hm.mul_(slot_valid)
    cx, cm = synth.device_tokens(gen, B * C, S, D, device)
    return (hx.reshape(B, H, S, D), hm.reshape(B, H, S, 1)), (cx.reshape(B, C, S, D), cm.reshape(B, C, S, 1))


def step(model, hist, cand):
    return model._forward(hist, cand)


def timed(fn, steps, warmup, dist_on, device="cuda"):
    """W untimed + EXACTLY `steps` timed calls bracketed by barrier + device sync on both sides; MAX over ranks."""
    on_gpu = torch.device(device).type == "cuda"
    sync = torch.cuda.synchronize if on_gpu else (lambda: None)
    for _ in range(warmup):
        fn()
    if dist_on:
        torch.distributed.barrier()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    sync()
    if dist_on:
        torch.distributed.barrier()
    dt = time.perf_counter() - t0
    if dist_on:
        t = torch.tensor([dt], dtype=torch.float64, device=device)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t.item())
    return dt


def count_ranks(device):
    """SUM all-reduce of ones over the process group: the number of ranks the collective library (RCCL) really
    joined.  Printed as `rccl_ranks` so a reader can tell an N-rank run from N copies of a 1-rank run."""
    t = torch.ones(1, dtype=torch.float32, device=device)
    torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.SUM)
    return int(round(float(t.item())))


def launch_ranks(args, argv):
    """`python bench.py --gpus N` with no torch.distributed.run environment: start the N ranks here.

    Runs BEFORE anything touches the GPU in this process (device_count() does not initialise it), starts one fresh
    child interpreter per GPU with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set (children, not an exec of this
    process), lets rank 0 print the one JSON line on the inherited stdout, and exits with the worst child code.  A
    rank that dies takes the others down (exact PIDs) instead of leaving them in a collective forever."""
    n = args.gpus
    if args.selftest_backend is None:
        have = torch.cuda.device_count()
        if have < n:
            print(f"bench.py: --gpus {n} requested but only {have} GPU(s) are visible; refusing to print an "
                  f"n_gpus={n} line from fewer devices", file=sys.stderr)
            return 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env))
    rc = 0
    alive = set(range(n))
    while alive:
        for r in sorted(alive):
            code = procs[r].poll()
            if code is None:
                continue
            alive.discard(r)
            if code != 0 and rc == 0:
                rc = code if code > 0 else 1
                print(f"bench.py: rank {r} exited with code {code}; stopping the other ranks", file=sys.stderr)
                for o in alive:
                    procs[o].terminate()
        time.sleep(0.05)
    return rc


def selftest_line(args, rank, world):
    """Launcher self-test (tests/test_bench_launcher.py): the rendezvous / barrier / MAX-over-ranks / rank-0-prints
    contract of this file over gloo on CPU with a stub step.  No hot-path work is done or claimed."""
    torch.distributed.init_process_group(args.selftest_backend, rank=rank, world_size=world)
    x = torch.randn(64, 64)
    dt = timed(lambda: x @ x, args.steps, args.warmup, True, device="cpu")
    ranks = count_ranks("cpu")
    if rank == 0:
        print(json.dumps({"metric": "launcher self-test (stub step, no hot-path work)", "value": world * args.steps / dt,
                          "unit": "stub steps/s", "n_gpus": world, "rccl_ranks": ranks, "steps": args.steps,
                          "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
                          "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "stub",
                          "config": {"workload": "none (launcher self-test)", "backend": args.selftest_backend}}))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def usable_cores():
    """Cores this process may actually use: affinity mask, capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(float(quota) / float(period))))
    except (OSError, ValueError):
        pass
    return max(1, min(n, 64))


def cpu_baseline(w, sd, sample_B=32, reps=10, warm=3, one_thread_B=4, one_thread_reps=3):
    """Oracle (torch CPU fp32 restatement, pinned to the reference by tests/golden) on the host cores: `warm` warm-up
    passes + `reps` timed passes over a `sample_B`-impression sample of the same workload shape with every usable core
    (BASELINE.md section 3), and a 1-thread line on a smaller sample (it is ~cores x slower)."""
    from oracle import xnrs_oracle as O
    threads = usable_cores()
    rng_batch = synth.make_batch(77, sample_B, w["H"], w["C"], w["S"], w["D"], min_len=5)
    hist = rng_batch["user_features"]["history"]["title_emb"]
    cand = rng_batch["candidate_features"]["title_emb"]
    sdc = {k: v.float().cpu() for k, v in sd.items()}

    def run(h, c, n_warm, n_rep):
        with torch.no_grad():
            for _ in range(n_warm):
                r = O.parent_forward(h, c, sdc, w["h"])
            t0 = time.perf_counter()
            for _ in range(n_rep):
                r = O.parent_forward(h, c, sdc, w["h"])
            return (time.perf_counter() - t0) / n_rep, r

    torch.set_num_threads(threads)
    dt, r = run(hist, cand, warm, reps)
    used = torch.get_num_threads()
    torch.set_num_threads(1)
    k = one_thread_B
    dt1, _ = run((hist[0][:k], hist[1][:k]), (cand[0][:k], cand[1][:k]), 1, one_thread_reps)
    torch.set_num_threads(threads)
    cpu = ""
    try:
        cpu = next(ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name"))
    except (OSError, StopIteration):
        pass
    shape = f"(H={w['H']},C={w['C']},S={w['S']},D={w['D']})"
    return dict(value=sample_B / dt, unit="impressions/s", cores=used, kind="port",
                sample=f"{sample_B} impressions of the same workload shape {shape}, {reps} timed passes after {warm} warm-ups, "
                       f"{dt:.2f} s/pass",
                one_thread=dict(value=k / dt1, unit="impressions/s", cores=1,
                                sample=f"{k} impressions {shape}, {one_thread_reps} timed passes after 1 warm-up, {dt1:.2f} s/pass"),
                cpu_model=cpu, logical_cpus=os.cpu_count()), r


def news_only_extra(device, steps=20, warmup=10):
    """BASELINE configs[1]: NRMS news encoder only, 1024 news, at the reference-valid stand-ins of the
    impossible 'd=300, 16 heads' (SURVEY.md finding 2) and at the shipped shape."""
    out = {}
    for name, (S, D, h) in {"S30_D300_h15": (30, 300, 15), "S30_D320_h16": (30, 320, 16), "S50_D768_h16": (50, 768, 16)}.items():
        w = dict(B=1, H=1, C=1, S=S, D=D, h=h, E=256 if D != 300 else 240, A=256)
        model, _ = build_model(w, device)
        gen = torch.Generator(device=device)
        gen.manual_seed(5)
        x, m = synth.device_tokens(gen, 1024, S, D, device)
        x, m = x.reshape(1, 1024, S, D), m.reshape(1, 1024, S, 1)
        fn = lambda: model.news_encoder((x, m))  # noqa: E731
        t_end = time.perf_counter() + 0.3  # let the clocks ramp after the idle CPU phase
        while time.perf_counter() < t_end:
            fn()
            torch.cuda.synchronize()
        dt = timed(fn, steps, warmup, False) / steps
        # EXECUTED FLOPs: the out-projection is folded behind the pooling on every path (the <= 32-token shapes inside the
        # single fused kernel, the 50 x 768 shape on the pipeline): one D x D product per news instead of one per token
        fl = 1024 * news_flops(S, D, 256, w["E"], folded=fold_on())
        fl_ref = 1024 * news_flops(S, D, 256, w["E"])
        out[name] = dict(news_per_s=1024 / dt, ms=dt * 1e3, tflops=fl / dt / 1e12,
                         frac_fp32_mfma=fl / dt / 1e12 / FP32_MFMA_PEAK_TFLOPS,
                         reference_order_tflops=fl_ref / dt / 1e12,  # the same news at the reference's operation order: not a utilisation
                         alg_gbs=1024 * (4 * S * D + 4 * S + 4 * w["E"] + 4) / dt / 1e9)
    return out


def other_model_flops(name, H, C, S=50, D=768, A=256, E=256):
    """Executed = algorithmic FLOPs per impression of the additive-only models (SURVEY.md section 8d formulas):
    StandardRec (standard_model.py:8-37): additive news tower + MLP head, additive user tower + MLP head;
    NAML (naml.py:61-112): two additive text towers + two 16->E category views + a 4-view additive pooler per news,
    additive user attention."""
    add = lambda n, d: 2 * n * d * A + 2 * n * A + 2 * n * d  # noqa: E731  fc1 + fc2 + weighted sum over n rows of width d
    news = add(S, D) + 2 * D * E + 2 * E * E
    if name == "standard":
        return (H + C) * news + add(H, E) + 4 * E * E + 2 * C * E
    return (H + C) * (2 * news + 2 * (2 * 16 * E) + add(4, E)) + add(H, E) + 2 * C * E


def other_models_extra(device, steps=5, warmup=2):
    """BASELINE configs[3]/[4] forward on one GPU: StandardRec (the CL bi-encoder, config/mind_small_CL.yml: additive-only
    towers + heads) and NAML (title + abstract + category views), B=512 impressions, H=25, C=5, S=50, D=768.  Per model:
    throughput, executed FLOPs against the fp32 matrix peak, the dominant kernel (fc1 + tanh + fc2-dot GEMM of the
    additive pooler) timed with hipEvents, and a parity spot-check of 4 impressions against the CPU oracle."""
    from oracle import xnrs_oracle as O
    out = {}
    B, H, C, S, D = 512, 25, 5, 50, 768
    gen = torch.Generator(device=device)
    gen.manual_seed(11)
    for name in ("standard", "NAML"):
        c = dict(model=name, E=256, bias=False, h=16, D=D, H=H, S=S)
        model = make_model(Cfg(synth.model_cfg(c)))
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        sd = synth.fill_state_dict(shapes, 99)
        model.load_state_dict(sd)
        model = model.eval().to(device)

        def toks(n):
            x, m = synth.device_tokens(gen, B * n, S, D, device)
            return x.reshape(B, n, S, D), m.reshape(B, n, S, 1)
        hist = {"title_emb": toks(H)}
        cand = {"title_emb": toks(C)}
        if name == "NAML":
            hist["abstract_emb"], cand["abstract_emb"] = toks(H), toks(C)
            for d_, n in ((hist, H), (cand, C)):
                d_["category_index"] = torch.randint(1, 20, (B, n), generator=gen, device=device, dtype=torch.int32)
                d_["subcategory_index"] = torch.randint(1, 301, (B, n), generator=gen, device=device, dtype=torch.int32)
        batch = {"user_features": {"history": hist, "other": {}}, "candidate_features": cand}
        fn = lambda: model(batch)  # noqa: E731
        dt = timed(fn, steps, warmup, False) / steps
        hip.profile_enable(hip.PROFILE_ALL)
        r = fn()
        torch.cuda.synchronize()
        st = hip.profile_read()
        hip.profile_enable(0)
        assert torch.isfinite(r).all(), name
        fl = other_model_flops(name, H, C) * B
        f_ms, f_n, f_fl = st["fc1_tanh_gemm"]

        def cut(v):
            if isinstance(v, torch.Tensor):
                return v[:4].cpu()
            if isinstance(v, dict):
                return {k: cut(x) for k, x in v.items()}
            return tuple(cut(x) for x in v) if isinstance(v, tuple) else v
        small = cut(batch)
        ref = O.naml_forward(small, sd) if name == "NAML" else O.parent_forward(
            small["user_features"]["history"]["title_emb"], small["candidate_features"]["title_emb"], sd, 16)
        err = (r[:4].cpu().double() - ref.double()).abs().max().item() / ref.abs().max().item()
        assert err <= 1e-4, (name, err)
        out[name] = dict(impressions_per_s=B / dt, ms=dt * 1e3, executed_tflops=fl / dt / 1e12,
                         frac_fp32_mfma=fl / dt / 1e12 / FP32_MFMA_PEAK_TFLOPS,
                         alg_gbs=B * (H + C) * (2 if name == "NAML" else 1) * (4 * S * D + 4 * S) / dt / 1e9,
                         stage_ms_per_step={k: round(v[0], 3) for k, v in st.items() if v[1]},
                         roofline={"bound": "mfma", "kernel": "additive_fused_kernel (one launch: fc1 + tanh + fc2 dot + pooling; gemm_f32_kernel<...RDOT> "
                                                                "+ additive_pool_kernel below its dispatch threshold)",
                                   "achieved": (f_fl / (f_ms * 1e-3) / 1e12) if f_ms > 0 else 0.0, "peak": FP32_MFMA_PEAK_TFLOPS,
                                   "unit": "TFLOP/s", "frac": (f_fl / (f_ms * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS) if f_ms > 0 else 0.0,
                                   "launches_timed": f_n, "avg_launch_ms": f_ms / max(f_n, 1), "traffic": None},
                         parity_max_rel_err_vs_cpu=err)
        tpath = os.path.join(ROOT, "profiles", "r04_traffic.json")
        if name == "standard" and os.path.exists(tpath):  # counter traffic of the history tower's launch (committed PMC summary)
            tj = json.load(open(tpath)).get("standard_fc1")
            if tj:
                out[name]["roofline"]["traffic"] = tj.get("hbm_bytes_per_launch")
                out[name]["roofline"]["traffic_source"] = {"file": "profiles/r04_traffic.json", "launch": tj.get("launch"),
                                                            "alg_bytes": tj.get("algorithmic_bytes_per_launch"), "note": tj.get("note")}
        if name == "standard":  # the same forward without the masked token rows (device-compacted encoder)
            model.news_encoder.unpadded = True
            try:
                dt_u = timed(fn, steps, warmup, False) / steps
                out[name]["unpadded"] = dict(impressions_per_s=B / dt_u, ms=dt_u * 1e3, equals_dense=bool(torch.equal(fn(), r)),
                                             masked_token_rows=1.0 - float(hist["title_emb"][1].mean().item()))
            finally:
                model.news_encoder.unpadded = False
    return out


def train_roofline(fn, dt):
    """Roofline entry of a grad step: EXECUTED matrix FLOPs of one step -- every GEMM / attention launch of the forward
    and the backward counted by the library's launch timer with the row counts it really ran over (the live-row paths
    contract over the unmasked token rows only) -- over the un-profiled step time `dt`, against the fp32 matrix peak;
    and the dominant kernel family of the backward, the weight-gradient GEMMs (dW = dY^T . X), from hipEvents around
    their launches (one extra, profiled step)."""
    hip.profile_enable(hip.PROFILE_ALL)
    fn()
    torch.cuda.synchronize()
    st = hip.profile_read()
    hip.profile_enable(0)
    total = sum(v[2] for v in st.values())
    w_ms, w_n, w_fl = st["bwd_dw_gemms"]
    ach = (w_fl / (w_ms * 1e-3) / 1e12) if w_ms > 0 else 0.0
    return {"bound": "mfma", "achieved": total / dt / 1e12, "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": total / dt / 1e12 / FP32_MFMA_PEAK_TFLOPS, "executed_gflop_per_step": total / 1e9,
            "what": "whole grad step: executed GEMM + attention FLOPs of forward and backward / step time (loss, optimizer and "
                    "pooling kernels carry no matrix work and count as time only)",
            "dominant_kernel": {"kernel": "weight-gradient GEMMs dW = dY^T.X (gemm_dw_kernel<KG> for live-row launches, "
                                          "gemm_f32_kernel<2,2,true,true,...> k-major otherwise)",
                                "achieved": ach, "frac": ach / FP32_MFMA_PEAK_TFLOPS, "launches_timed": w_n,
                                "avg_launch_ms": w_ms / max(w_n, 1), "alg_flops_per_launch": w_fl / max(w_n, 1), "traffic": None},
            "stage_ms_profiled_step": {k: round(v[0], 3) for k, v in st.items() if v[1]},
            "stage_tflops": {k: (v[2] / (v[0] * 1e-3) / 1e12) for k, v in st.items() if v[0] > 0}}


TRAIN_W = dict(B=64, H=25, C=5, S=50, D=768, h=16, E=256, A=256)
TRAIN_MODELS = {"nrms": "NRMS", "standard": "standard", "naml": "NAML"}


class _StubRec(torch.nn.Module):
    """Launcher self-test only (--selftest-backend gloo --train ...): a CPU stand-in with ParentRec's two entry points, so
    that the data-parallel plumbing of the training line (weight broadcast, shard layout, embedding all-gather, gradient
    bucket all-reduce, the JSON line) runs without a GPU.  No hot-path work is done or claimed."""

    def __init__(self, d, e):
        super().__init__()
        self.news = torch.nn.Linear(d, e)
        self.user = torch.nn.Linear(e, e)

    def _vec(self, feat):
        x, m = feat
        return self.news((x * m).sum(2) / (m.sum(2) + 1e-8))

    def get_user_embeddings(self, batch):
        return self.user(self._vec(batch["user_features"]["history"]["title_emb"]).mean(1))

    def forward(self, batch):
        u = self.get_user_embeddings(batch)
        c = self._vec(batch["candidate_features"]["title_emb"])
        return torch.bmm(c, u.unsqueeze(2))


def make_train_job(model_name, device, seed=7, dist_factory=None, stub=False):
    """Model, synthetic batch and the grad step of the reference (ContrastiveRankingTrainer._train_step,
    training.py:402-431) IN THE REFERENCE'S CALL ORDER: preds = model(batch) -> relu/MSE (training.py:388-392); user
    embeddings = model.get_user_embeddings(batch), i.e. a SECOND history encode (training.py:409, parent.py:49-81); InfoNCE
    on them; backward; Adam.  What the library shares between the two encodes is its business and exact: the Q|K|V
    projection and one dW product per projection for NRMS (the attention-dropout draws differ), the whole deterministic
    encode for StandardRec / NAML (no dropout anywhere: bit-identical outputs; tests/test_hip_train_step.py).
    dist_factory: None, or model -> (distributed module, ShardLayout, GradBucket, n_global) for the data-parallel job."""
    w = TRAIN_W
    name = TRAIN_MODELS.get(model_name, model_name)
    if stub:  # launcher self-test on CPU: tiny shapes, a stand-in model and a stand-in for the fused InfoNCE
        w = dict(w, B=4, H=3, C=2, S=4, D=8, E=8)
        name = "stub"
        torch.manual_seed(1234)
        model = _StubRec(w["D"], w["E"]).to(device)

        def infonce(e, labels, t):
            return (e @ e.t() / t).logsumexp(1).mean()
    else:
        from xnrs_amd.losses import contrastive_loss as infonce  # fused HIP forward/backward (training.py:433-472)
        model, _ = build_model(w, device, model_name=name)
    model.train()
    dist = dist_factory(model) if dist_factory is not None else None
    # the reference's optimizer (training.py:39: torch.optim.Adam(model.parameters(), lr)); `fused` is torch's one-kernel
    # implementation of the same update (the default "foreach" form is ~8 launches per step)
    try:
        opt = torch.optim.Adam(model.parameters(), lr=1e-4, fused=not stub)
    except (RuntimeError, TypeError):
        opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    B, H, C, S, D = w["B"], w["H"], w["C"], w["S"], w["D"]
    if stub:
        g = torch.Generator().manual_seed(seed)
        hist = (torch.randn(B, H, S, D, generator=g), torch.ones(B, H, S, 1))
        cand = (torch.randn(B, C, S, D, generator=g), torch.ones(B, C, S, 1))
    else:
        hist, cand = make_inputs(w, device, seed=seed)
    hfeat, cfeat = {"title_emb": hist}, {"title_emb": cand}
    if name == "NAML":  # title + abstract token tensors, category / subcategory ids (naml.py:61-112)
        gen = torch.Generator(device=device)
        gen.manual_seed(seed + 1)
        ah, ac = make_inputs(w, device, seed=seed + 2)
        # an empty history slot is empty in every view (dataset.py:82-85)
        slot = hist[1].reshape(B, H, S).ne(0).any(dim=2).to(torch.float32)
        hfeat["abstract_emb"] = (ah[0] * slot[:, :, None, None], ah[1] * slot[:, :, None, None])
        cfeat["abstract_emb"] = ac
        for d_, n in ((hfeat, H), (cfeat, C)):
            d_["category_index"] = torch.randint(1, 20, (B, n), generator=gen, device=device, dtype=torch.int32)
            d_["subcategory_index"] = torch.randint(1, 301, (B, n), generator=gen, device=device, dtype=torch.int32)
    targets = torch.zeros(B, C, 1, device=device)
    targets[:, 0] = 1.0
    gen = torch.Generator(device=device)
    gen.manual_seed(seed + 1000)
    labels = torch.randint(0, 6, (B,), device=device, generator=gen)
    batch = {"user_features": {"history": hfeat, "other": {}}, "candidate_features": cfeat}
    w_ = w  # (the closure below reads the job's own shapes)

    def fn(step_opt=True):
        if dist is not None:
            dist[2].zero_grad()
        else:
            opt.zero_grad()
        preds = torch.relu(model(batch))
        rec = torch.nn.functional.mse_loss(preds, targets)
        ue = model.get_user_embeddings(batch)  # the reference's second history encode
        ue = ue.reshape(ue.size(0), -1)
        if dist is not None:  # two collectives, no host sync: [embedding | label bits] all-gather + flat gradient all-reduce
            D_, layout, bucket, n_global = dist
            ue_all, lab_all = D_.gather_embeddings_and_labels(ue, labels, layout)
            loss = D_.global_train_loss(rec, w_["B"], n_global, infonce(ue_all, lab_all, 0.08), 0.1)
        else:
            loss = rec + 0.1 * infonce(ue, labels, 0.08)
        loss.backward()
        if dist is not None:
            dist[2].allreduce()
        if step_opt:
            opt.step()
        return loss
    return model, opt, batch, targets, labels, fn


def graph_train_step(model, fn, device, steps, warmup):
    """The same grad step captured ONCE in a hipGraph (forward + losses + backward + Adam) and replayed: possible because
    the step has no host synchronisation (row lists and their counts stay on the device).  Attention dropout draws a fresh
    mask per replay through a device seed word incremented inside the captured step (ops.set_dropout_seed_word)."""
    from xnrs_amd import ops
    opt = torch.optim.Adam(model.parameters(), lr=1e-4, capturable=True)
    word = torch.zeros(1, dtype=torch.int64, device=device)
    ops.set_dropout_seed_word(word)
    try:
        def one():
            word.add_(1)
            opt.zero_grad(set_to_none=False)
            loss = fn(step_opt=False)
            opt.step()
            return loss
        for p in model.parameters():
            if p.requires_grad:
                p.grad = torch.zeros_like(p)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                one()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):  # (the warm-up stream: see tests/test_hip_train_step.py on AccumulateGrad streams)
            loss = one()
        dt = timed(g.replay, steps, warmup, False) / steps
        return dict(ms=dt * 1e3, loss_finite=bool(torch.isfinite(loss).item()))
    finally:
        ops.set_dropout_seed_word(None)


def train_step_extra(device, steps=20, warmup=5, model_name="NRMS", variants=True):
    """The grad step of the reference (training.py:402-431) on the HIP path at the shipped config (batch 64, H=25, C=5,
    S=50, D=768, train mode: NRMS attention dropout 0.1): see make_train_job."""
    from xnrs_amd import autograd as AG
    from xnrs_amd.losses import contrastive_loss as infonce
    w = TRAIN_W
    model, opt, batch, targets, labels, fn = make_train_job(model_name, device)
    stats0 = dict(AG.STATS)
    dt = timed(fn, steps, warmup, False) / steps
    per_step = {k: (AG.STATS[k] - stats0[k]) / (steps + warmup) for k in AG.STATS}
    out = dict(ms=dt * 1e3, impressions_per_s=w["B"] / dt, batch=w["B"], loss_finite=bool(torch.isfinite(fn()).item()),
               step="reference order: model(batch) + get_user_embeddings(batch) (two history encodes), MSE + 0.1 InfoNCE, backward, Adam",
               host_syncs_in_step=0 if per_step["device_list_forwards"] > 0 or per_step["live_row_forwards"] == 0 else "one per encoder call",
               per_step=per_step)
    assert out["loss_finite"], model_name
    out["roofline"] = train_roofline(fn, dt)
    if not variants:
        return out
    try:
        out["hipgraph_replay"] = graph_train_step(model, fn, device, steps, warmup)
    except Exception as e:  # noqa: BLE001  (reported, never hidden)
        out["hipgraph_replay"] = {"error": f"{type(e).__name__}: {e}"[:300]}
    if TRAIN_MODELS.get(model_name, model_name) != "NRMS":
        # what the sharing of the deterministic second encode saves: the same step computing both encodes
        old, AG.SHARE_OUTPUTS = AG.SHARE_OUTPUTS, False
        try:
            dt2 = timed(fn, steps, warmup, False) / steps
            out["both_encodes_computed"] = dict(ms=dt2 * 1e3, impressions_per_s=w["B"] / dt2)
        finally:
            AG.SHARE_OUTPUTS = old
        return out
    # NOT the reference's step (labelled extra): one history encode feeding both the scores and the InfoNCE term
    # (forward(..., return_embeddings=True) instead of the second encode at training.py:409 -- one dropout draw instead of two)
    def fn_shared():
        opt.zero_grad()
        r, u, _ = model(batch, return_embeddings=True)
        loss = torch.nn.functional.mse_loss(torch.relu(r), targets) + 0.1 * infonce(u.squeeze(1), labels, 0.08)
        loss.backward()
        opt.step()
        return loss
    dt3 = timed(fn_shared, steps, warmup, False) / steps
    out["one_history_encode_NOT_the_reference_step"] = dict(ms=dt3 * 1e3, impressions_per_s=w["B"] / dt3)
    # the round-3 step for comparison: host-built row lists (one .tolist() per encoder call), one dW product per encode
    old = (AG.DEVICE_LISTS, AG.MERGE_DW)
    AG.DEVICE_LISTS, AG.MERGE_DW = False, False
    try:
        dt4 = timed(fn, steps, warmup, False) / steps
        out["round3_path_host_lists_unmerged_dw"] = dict(ms=dt4 * 1e3, impressions_per_s=w["B"] / dt4)
    finally:
        AG.DEVICE_LISTS, AG.MERGE_DW = old
    return out


def ig_step_extra(device, n_steps=40):
    """The ONE timing the reference publishes for this code: integrated-gradient steps per second --
    per step a forward of one impression (H history news, 1 candidate, S=50, D=768) and autograd.grad(score, history
    tokens), Explainer.explain_score_in_batch (xnrs/explain.py:144-166), through the HIP input-gradient path.  Reference
    figures (an unnamed CUDA device, context only): 316.7 it/s (9-news history), 177.4 it/s (one MIND session)."""
    out = {"reference_unnamed_cuda": {"H9": 316.70, "mind_session": 177.41, "source": "BASELINE.md section 1"}}
    for name in ("standard", "NRMS"):
        for H in (9, 25):
            w = dict(B=1, H=H, C=1, S=50, D=768, h=16, E=256, A=256)
            model, _ = build_model(w, device, model_name=name)
            (hx, hm), (cx, cm) = make_inputs(w, device, seed=50 + H, full_history=True)
            hx = hx.clone().requires_grad_()
            hm = hm.clone().requires_grad_()   # explain.py:152 marks the mask too
            cx = cx.clone().requires_grad_()
            cm = cm.clone().requires_grad_()

            def run(n):
                c, _ = model.news_encoder((cx, cm))
                da = 1.0 / n
                grads = []
                for a in torch.arange(da, 1 + da, da)[:n]:
                    ga = a * hx
                    ha, ham = model.news_encoder((ga, hm))
                    ua = model.user_encoder.forward(inpt=(ha, ham))
                    sa = torch.relu(model.rec_model(ua, c))
                    grads.append(torch.autograd.grad(sa, ga)[0])
                return torch.cat(grads)
            run(5)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g = run(n_steps)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            out[f"{name}_H{H}"] = dict(it_per_s=n_steps / dt, ms_per_it=dt / n_steps * 1e3, grads_finite=bool(torch.isfinite(g).all().item()))
            # the same explanation with its interpolation steps as the batch dimension (xnrs_amd/explain.py): one forward +
            # one input-gradient pass over all 100 scaled copies of the history, the same attributions
            from xnrs_amd.explain import integrated_gradients
            NS = 100
            args = (model, hx.detach(), hm.detach(), cx.detach(), cm.detach())
            integrated_gradients(*args, n_steps=NS)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                res = integrated_gradients(*args, n_steps=NS)
            torch.cuda.synchronize()
            dtb = (time.perf_counter() - t0) / 3
            out[f"{name}_H{H}"]["batched_100_steps"] = dict(
                it_per_s=NS / dtb, ms_per_explanation=dtb * 1e3, attr_finite=bool(torch.isfinite(res["attr"]).all().item()),
                what="all 100 interpolation steps of explain.py:160-166 as ONE batch (steps are independent): same attributions")
    return out


def eval_epoch_extra(device, n_news=20000, n_sess=20000):
    """Evaluation path (xnrs_amd/evaluation.py): encode every news of a resident table ONCE, then score
    impressions as CSR candidate lists + per-impression metrics on the device.  The reference's test loop
    (training.py:61-67,194-243) runs batch_size 1 and re-encodes all candidates of every impression."""
    import numpy as np
    from xnrs_amd.data import Behaviors, NewsStore
    from xnrs_amd.evaluation import evaluate
    w = dict(B=1, H=25, C=5, S=50, D=768, h=16, E=256, A=256)
    model, _ = build_model(w, device)
    gen = torch.Generator(device=device)
    gen.manual_seed(21)
    x, m = synth.device_tokens(gen, n_news + 1, w["S"], w["D"], device)
    x[0] = 0
    m[0] = 0
    store = NewsStore(x, m.reshape(n_news + 1, w["S"]), list(range(n_news)))
    rng = np.random.default_rng(3)

    def csr(lo, hi):
        cnt = rng.integers(lo, hi + 1, size=n_sess)
        off = np.zeros(n_sess + 1, dtype=np.int64)
        np.cumsum(cnt, out=off[1:])
        return torch.from_numpy(off).to(device), torch.from_numpy(rng.integers(1, n_news + 1, size=int(off[-1])).astype(np.int32)).to(device)
    beh = Behaviors(csr(1, 40), csr(1, 3), csr(5, 60), ["t"] * n_sess)
    beh.theme_labels = beh.theme_labels.to(device)
    evaluate(model, store, beh, w["H"], batch=8192)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = evaluate(model, store, beh, w["H"], batch=8192)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    # the same epoch with the padding-free news encoder (exact; section 10.1 of DESIGN.md)
    model.news_encoder.unpadded = True
    try:
        evaluate(model, store, beh, w["H"], batch=8192)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res_u = evaluate(model, store, beh, w["H"], batch=8192)
        torch.cuda.synchronize()
        dt_u = time.perf_counter() - t0
    finally:
        model.news_encoder.unpadded = False
    return dict(n_news=n_news, n_impressions=n_sess, candidates=int(beh.pos_off[-1] + beh.neg_off[-1]), seconds=dt,
                impressions_per_s=n_sess / dt, auc=res["auc"],
                unpadded=dict(seconds=dt_u, impressions_per_s=n_sess / dt_u, same_metrics=bool(res_u == res)))


def store_upload_extra(device, n_news=4096):
    """File -> HBM loader (NewsStore.load_to_device, replaces the pandas-pickle load of xnrs/data/mind.py:161-164): a
    `n_news` x 50 x 768 fp32 store written to a RAM-backed temp dir (so the figure is the loader's pipeline -- memory map
    -> two pinned staging buffers -> HBM -- not a disk), loaded twice (the second pass has warm page cache and pinned
    pools), checked against the source."""
    import shutil
    import tempfile
    from xnrs_amd.data import NewsStore
    w = WORKLOAD
    gen = torch.Generator(device=device)
    gen.manual_seed(41)
    tx, tm = synth.device_tokens(gen, n_news + 1, w["S"], w["D"], device)
    store = NewsStore(tx, tm.reshape(n_news + 1, w["S"]), list(range(n_news)))
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    d = tempfile.mkdtemp(prefix="xnrs_store_", dir=base)
    try:
        path = os.path.join(d, "news")
        store.save(path)
        out = {}
        for name in ("first_load", "second_load"):
            st = {}
            loaded = NewsStore.load_to_device(path, device, rows_per_chunk=1024, stats=st)
            torch.cuda.synchronize()
            out[name] = {"gb_per_s": st["gb_per_s"], "seconds": st["seconds"], "bytes": st["bytes"]}
        out["equals_source"] = bool(torch.equal(loaded.x, store.x) and torch.equal(loaded.m, store.m))
        out["where"] = "RAM-backed temp dir" if base else "temp dir on disk"
        out["rows_per_chunk"] = 1024
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def gather_roofline(device, n_news=16384, n=512 * 55, reps=5):
    """The gather stage as its own kernel (xnrs_gather_rows: out[i] = table[ids[i]] for whole 150-KB news blocks, what
    NewsRecDataset.__getitem__ + torch.cat do on the host): HBM-bound, timed live with events on the launching stream.
    Algorithmic bytes = rows read + rows written.  The counter view (FETCH_SIZE x2 / WRITE_SIZE) of the same kernel on the
    65 536-news table is profiles/r02_gather_rocprof.txt; inside the encoders the gather is folded into the first GEMM's
    loads instead (extra.id_path_B512)."""
    import numpy as np
    from xnrs_amd.data import NewsStore
    w = WORKLOAD
    gen = torch.Generator(device=device)
    gen.manual_seed(31)
    tx, tm = synth.device_tokens(gen, n_news + 1, w["S"], w["D"], device)
    store = NewsStore(tx, tm.reshape(n_news + 1, w["S"]), list(range(n_news)))
    rng = np.random.default_rng(5)
    out = {"bound": "hbm", "peak": HBM_PEAK_GBS, "unit": "GB/s", "kernel": "gather_rows_kernel<true>",
           "table": f"{n_news} news x {w['S']} x {w['D']} fp32 ({(n_news + 1) * w['S'] * w['D'] * 4 / 1e9:.1f} GB)", "rows": n}
    row_bytes = w["S"] * w["D"] * 4
    for dist in ("uniform", "zipf1.1"):
        ids = rng.integers(1, n_news + 1, size=n) if dist == "uniform" else np.minimum(rng.zipf(1.1, size=n), n_news)
        ids = torch.from_numpy(ids.astype(np.int32)).to(device)
        x = torch.empty((n, w["S"], w["D"]), dtype=torch.float32, device=device)
        st = hip.stream_ptr(device)

        def go():
            hip.check(hip.lib().xnrs_gather_rows(hip.ptr(store.x), hip.ptr(ids), hip.ptr(x), n, w["S"] * w["D"], st), "xnrs_gather_rows")
        go()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            go()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        gbs = 2.0 * n * row_bytes / (ms * 1e-3) / 1e9
        out[dist] = {"achieved": gbs, "frac": gbs / HBM_PEAK_GBS, "avg_launch_ms": ms, "alg_bytes_per_launch": 2 * n * row_bytes,
                     "distinct_rows": int(torch.unique(ids).numel())}
        del x
    out["achieved"], out["frac"] = out["uniform"]["achieved"], out["uniform"]["frac"]
    out["traffic"] = None
    for tname in ("r04_traffic.json", "r03_traffic.json", "r02_traffic.json"):
        tpath = os.path.join(ROOT, "profiles", tname)
        if os.path.exists(tpath):
            tj = json.load(open(tpath))
            out["traffic"] = tj.get("gather_rows_hbm_bytes_per_launch")  # null when that round's gather run was not profiled
            out["traffic_source"] = {"file": "profiles/" + tname, "commit": tj.get("commit"), "date": tj.get("date"),
                                     "note": tj.get("gather_note")}
            break
    return out


def id_path_extra(device, steps=5, warmup=2, n_news=65536):
    """The device-resident news table path (ParentRec.forward_ids): B=512 impressions given as row ids into a
    65 536-news table (10 GB, MIND-small scale), ids ~ Zipf(1.1); the gather happens in the
    first GEMM's load.  `dedup` encodes each distinct news of the step once -- less algorithmic work, hence
    reported separately from the headline value."""
    import numpy as np
    w = WORKLOAD
    model, _ = build_model(w, device)
    gen = torch.Generator(device=device)
    gen.manual_seed(31)
    tx, tm = synth.device_tokens(gen, n_news + 1, w["S"], w["D"], device)
    tx[0] = 0
    tm[0] = 0
    tm = tm.reshape(n_news + 1, w["S"])
    rng = np.random.default_rng(5)
    z = np.minimum(rng.zipf(1.1, size=(w["B"], w["H"] + w["C"])), n_news).astype(np.int32)
    n_hist = rng.integers(1, w["H"] + 1, size=(w["B"], 1))
    z[:, :w["H"]][np.arange(w["H"])[None, :] >= n_hist] = 0  # empty history slots
    ids = torch.from_numpy(z).to(device)
    hist_ids, cand_ids = ids[:, :w["H"]].contiguous(), ids[:, w["H"]:].contiguous()
    out = {"table_news": n_news, "distinct_ids_in_step": int(torch.unique(ids).numel()), "ids_in_step": int(ids.numel())}
    for name, dd in (("gather", False), ("gather_dedup", True)):
        fn = lambda: model.forward_ids(tx, tm, hist_ids, cand_ids, dedup=dd)  # noqa: E731
        dt = timed(fn, steps, warmup, False) / steps
        out[name] = dict(impressions_per_s=w["B"] / dt, ms=dt * 1e3)
    r0 = model.forward_ids(tx, tm, hist_ids, cand_ids)
    r1 = model.forward_ids(tx, tm, hist_ids, cand_ids, dedup=True)
    out["dedup_equals_plain"] = bool(torch.equal(r0, r1))
    return out


def gemm_modes_extra(model, hist, cand, steps, scores_f32, cpu_sample):
    """The same step with the forward GEMMs on the bf16 matrix cores by operand splitting (opt-in modes 1 and 2):
    throughput, per-stage time, distance of the scores to the fp32-MFMA scores of the headline run (full batch)
    and, when the CPU baseline ran, to the CPU oracle on its sample."""
    out = {}
    B = hist[0].shape[0]
    for mode in (1, 2):
        hip.set_gemm_mode(mode)
        fn = lambda: step(model, hist, cand)  # noqa: E731
        dt = timed(fn, steps, 2, False)
        hip.profile_enable(hip.PROFILE_ALL)
        r = fn()
        torch.cuda.synchronize()
        st = hip.profile_read()
        hip.profile_enable(0)
        e = {"impressions_per_s": B * steps / dt, "ms_per_step": dt / steps * 1e3,
             "stage_ms_per_step": {k: round(v[0], 3) for k, v in st.items()},
             "qkv_gemm_alg_tflops": st["qkv_gemm"][2] / (st["qkv_gemm"][0] * 1e-3) / 1e12,
             "max_rel_diff_vs_f32_mfma_scores": ((r - scores_f32).abs().max() / scores_f32.abs().max()).item()}
        if cpu_sample is not None:
            b, ref = cpu_sample
            got = model._forward(b["user_features"]["history"]["title_emb"], b["candidate_features"]["title_emb"])
            e["parity_max_rel_err_vs_cpu"] = (got.cpu().double() - ref.double()).abs().max().item() / ref.abs().max().item()
        out[GEMM_MODES[mode][0].split(" via ")[1].split(" ")[0]] = e
    hip.set_gemm_mode(0)
    return out


def unfolded_extra(model, hist, cand, steps, scores):
    """The same step with the reference's operation order (per-token out-projection, XNRS_FOLD_OUT=0): what the folded
    out-projection buys, and how far the two score sets are apart."""
    with hip.knobs(XNRS_FOLD_OUT="0"):
        fn = lambda: step(model, hist, cand)  # noqa: E731
        dt = timed(fn, steps, 2, False)
        r = fn()
    B = hist[0].shape[0]
    return dict(impressions_per_s=B * steps / dt, ms_per_step=dt / steps * 1e3,
                max_rel_diff_vs_folded=((r - scores).abs().max() / scores.abs().max()).item())


def padding_free_extra(model, hist, cand, steps, scores_dense):
    """The same step without the padding work (both exact, both data-dependent, hence not the headline):
      skip_empty : all-masked news -- the empty history slots, 49 % of this synthetic workload's history
                   (history length ~ U{1..H}) -- take the constant head(0) vector;
      unpadded   : masked TOKEN rows (token length ~ U{5..S}: 45 % of the rows) are skipped wherever they cannot
                   reach the output (Q projection, attention rows, out-projection, fc1, pooling; K/V stay dense)."""
    B, H = hist[1].shape[:2]
    enc = model.news_encoder
    out = {"empty_history_slots": 1.0 - hist[1].reshape(B, H, -1).ne(0).any(dim=2).float().mean().item(),
           "masked_token_rows_of_live_news": None}
    live = hist[1].reshape(B * H, -1).ne(0)
    nz = live.any(dim=1)
    n_tok = float(nz.sum().item() * live.shape[1] + cand[1].numel())
    out["masked_token_rows_of_live_news"] = 1.0 - float(live[nz].sum().item() + cand[1].ne(0).sum().item()) / n_tok
    from xnrs_amd import ops
    out["how"] = ("unpadded / skip_empty+unpadded: row lists and counts built on the device (xnrs_text_encoder_fwd_compact): "
                  "no host read, hipGraph-capturable, all-masked news dropped by the same lists; "
                  "skip_empty+unpadded_host_lists: the round-2 path (one nonzero per switch and encoder call)")
    for name, flags in (("skip_empty", dict(skip_empty=True)), ("unpadded", dict(unpadded=True)),
                        ("skip_empty+unpadded", dict(skip_empty=True, unpadded=True)),
                        ("skip_empty+unpadded_host_lists", dict(skip_empty=True, unpadded=True))):
        for k, v in flags.items():
            setattr(enc, k, v)
        on_device = ops.COMPACT_ON_DEVICE
        if name.endswith("host_lists"):
            ops.COMPACT_ON_DEVICE = False
        try:
            fn = lambda: step(model, hist, cand)  # noqa: E731
            dt = timed(fn, steps, 2, False)
            r = fn()
            same = bool(torch.equal(r, scores_dense))
            diff = ((r - scores_dense).abs().max() / scores_dense.abs().max()).item()
        finally:
            enc.skip_empty = enc.unpadded = False
            ops.COMPACT_ON_DEVICE = on_device
        # (in the split GEMM modes a launch of fewer than 512 tiles runs on the fp32 kernel, so a different pass
        # size can move a result by fp32 rounding noise; in the default mode the scores are bitwise equal)
        out[name] = dict(impressions_per_s=B * steps / dt, ms_per_step=dt / steps * 1e3, equals_dense=same,
                         max_rel_diff_vs_dense=diff)
    return out


def latency_extra(device, reps=50):
    """Launch-bound regime: ONE impression (H=25, C=5, S=50, D=768) -- ~15 kernel launches -- eager vs a
    captured hipGraph replay (the C ABI allocates nothing and syncs nothing, so the forward is capturable)."""
    w = dict(B=1, H=25, C=5, S=50, D=768, h=16, E=256, A=256)
    model, _ = build_model(w, device)
    hist, cand = make_inputs(w, device, seed=3)
    fn = lambda: model._forward(hist, cand)  # noqa: E731
    # (best of three: the eager loop is bound by ~30 host-side launches per call, and a busy host core shows up as a
    # several-fold outlier that says nothing about the path)
    eager = min(timed(fn, reps, 10, False) / reps for _ in range(3))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    graph = timed(g.replay, reps, 10, False) / reps
    # the same request with history and candidates as TWO news-encoder calls (the reference's order; bit for bit the same scores)
    cap = type(model).ONE_CALL_MAX_BYTES
    try:
        model.ONE_CALL_MAX_BYTES = 0
        two = min(timed(fn, reps, 10, False) / reps for _ in range(3))
    finally:
        model.ONE_CALL_MAX_BYTES = cap
    return dict(eager_ms=eager * 1e3, hipgraph_ms=graph * 1e3, two_news_encoder_calls_ms=two * 1e3)


def train_scaling(args, device, rank, world, dist_on):
    """--train: the grad step of the reference (training.py:402-431, in its call order: make_train_job) as a data-parallel
    job.  Weak scaling: every rank owns 64 impressions (mind_small_NRMS.yml batch size; mind_small_CL.yml uses 16 -- too
    little work per GPU), weights replicated.  Per step: local forward + second history encode,
    relu/MSE on the local impressions, InfoNCE over the GLOBAL batch (differentiable all-gather of the user embeddings +
    labels), backward, one flat SUM all-reduce of the gradients, Adam."""
    from xnrs_amd import distributed as D
    stub = args.selftest_backend is not None  # launcher self-test: CPU stand-in model over gloo (tests/test_bench_launcher.py)
    w = dict(TRAIN_W, B=4) if stub else TRAIN_W
    n_global = w["B"] * (world if dist_on else 1)
    # once per run: weights broadcast from rank 0, the shard layout (fixed per-rank batch -> no communication) and the
    # persistent gradient bucket
    def factory(model):
        D.broadcast_parameters(model)
        # --overlap-buckets: one bucket per tower, all-reduced asynchronously as each completes during the backward
        # (xnrs_amd.distributed.OverlappedGradBuckets); default: ONE flat bucket reduced after the backward
        bucket = D.OverlappedGradBuckets.by_tower(model) if args.overlap_buckets else D.GradBucket(model.parameters())
        return (D, D.ShardLayout.uniform(w["B"]), bucket, n_global)
    model, opt, batch, targets, labels, fn = make_train_job(args.train, device, seed=2000 + rank,
                                                            dist_factory=factory if dist_on else None, stub=stub)
    dt = timed(fn, args.steps, args.warmup, dist_on, device=device)
    n_gpus = world if dist_on else 1
    # every rank runs the profiled step (it contains the collectives)
    roof = None if stub else train_roofline(fn, dt / args.steps)
    return {"roofline": roof, "metric": "train impressions/sec (forward + second history encode + loss + backward + gradient all-reduce + Adam)",
            "value": n_global * args.steps / dt, "unit": "impressions/s", "n_gpus": n_gpus, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": GEMM_MODES[args.gemm_mode][0], "data": "stub" if stub else "synthetic",
            "build_id": None if stub else hip.build_id(),
            "config": {"workload": f"{args.train} grad step in the reference's call order (model(batch) + get_user_embeddings(batch): "
                                   "two history encodes, training.py:402-431), 64 impressions per GPU (H=25, C=5, S=50, D=768), global "
                                   "in-batch InfoNCE (lambda 0.1, tau 0.08), train mode (NRMS: attention dropout 0.1)",
                       "parallelism": f"impressions sharded over {n_gpus} GPU(s); per step ONE all-gather of (64, 256+1) [user "
                                      "embedding | label bits] + " + ("one asynchronous fp32 gradient all-reduce per tower, overlapped "
                                      "with the backward" if args.overlap_buckets else "ONE flat fp32 gradient all-reduce in a "
                                      "persistent bucket") + ", no host sync"},
            "loss_finite": bool(torch.isfinite(fn()).item())}


def qkv_roofline(prof, w, gemm_mode):
    """--full: roofline entry of the dominant kernel (the fused Q/K/V projection) from the launch timer that ran during the
    timed steps (`prof` = hip.profile_read() of stage 0)."""
    mode_products = GEMM_MODES[gemm_mode][1]
    q_ms, q_n, q_fl = prof["qkv_gemm"]
    ach = (q_fl / max(q_n, 1)) / (q_ms / max(q_n, 1) * 1e-3) / 1e12 if q_n else 0.0
    # `traffic` cannot be measured in this run (PMC counters need rocprofv3 around the process): it is read from the
    # committed PMC summary of the SAME kernel and launch shape and labelled with where and when that was taken
    # The counters were taken on ONE launch shape -- a full 65 500-row pass -- so `traffic` sits next to the algorithmic
    # bytes of THAT launch (`traffic_launch`), not next to the mean over this run's mixed launches; null when the file
    # does not say which launch it measured.
    traffic, traffic_source = None, None
    for tname in ("r04_traffic.json", "r03_traffic.json", "r02_traffic.json"):
        tpath = os.path.join(ROOT, "profiles", tname)
        if os.path.exists(tpath):
            tj = json.load(open(tpath))
            launch = tj.get("qkv_launch") or ({"rows": 65500, "grid_threads": 2359296} if "65 500-row pass" in str(tj.get("kernel")) else None)
            if launch is None:
                continue
            traffic = tj.get("qkv_gemm_hbm_bytes_per_launch")
            traffic_source = {"file": "profiles/" + tname, "commit": tj.get("commit"), "date": tj.get("date"),
                              "kernel": tj.get("kernel"), "method": tj.get("method", "rocprofv3 --pmc, FETCH_SIZE x2 + WRITE_SIZE, separate passes"),
                              "traffic_launch": dict(launch, alg_bytes=tj.get("algorithmic_bytes_per_launch"),
                                                     note="the counters belong to this launch shape: compare `traffic` with ITS "
                                                          "alg_bytes; roofline.alg_bytes_per_launch is the mean over this run's launches "
                                                          "(the last pass of every call is shorter)")}
            break
    # modes 1/2 issue `mode_products` bf16 MFMA products per algorithmic fp32 product: achieved = issued
    # matrix flops against the dense bf16 peak
    return {"bound": "mfma", "achieved": ach * mode_products,
            "peak": FP32_MFMA_PEAK_TFLOPS if gemm_mode == 0 else BF16_MFMA_PEAK_TFLOPS,
            "unit": "TFLOP/s",
            "frac": ach * mode_products / (FP32_MFMA_PEAK_TFLOPS if gemm_mode == 0 else BF16_MFMA_PEAK_TFLOPS),
            "traffic": traffic if gemm_mode == 0 else None,
            "traffic_source": traffic_source if gemm_mode == 0 else None,
            "alg_bytes_per_launch": (q_fl / max(q_n, 1)) / (6.0 * w["D"] * w["D"]) * (4 * w["D"] + 12 * w["D"]),
            "kernel": ("gemm_f32_kernel<2,2,...> (fused Q/K/V projection)" if gemm_mode == 0 else
                       f"gemm_split_kernel<{4 - gemm_mode},...> (fused Q/K/V projection)"),
            "alg_tflops": ach,
            "launches_timed": q_n, "avg_launch_ms": q_ms / max(q_n, 1),
            "alg_flops_per_launch": q_fl / max(q_n, 1)}


def dump_outputs(d, arrays, rank=0):
    """--dump-outputs: `arrays` ({name: tensor}, what a caller of the timed path receives) as d/<name>.npy in float32
    (d/<name>_rank<r>.npy on rank r > 0), 64 MB at most in all."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    host = {k: v.detach().to(torch.float32).cpu().numpy() for k, v in arrays.items()}
    total = sum(a.nbytes for a in host.values())
    assert total <= 64 << 20, f"--dump-outputs: {total} bytes > 64 MB"
    for k, a in host.items():
        np.save(os.path.join(d, k + (f"_rank{rank}" if rank else "") + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: the roofline of the dominant kernel (launch timer on during the timed "
                         "steps), the fully-live batch, the gather roofline, the CPU baseline with its parity check and the "
                         "extras; off (default): set up, warm up, time the steps, write --dump-outputs, print the line")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip the extras")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the scores of the last timed step as DIR/scores.npy (float32; "
                         "rank r > 0: DIR/scores_rank<r>.npy)")
    ap.add_argument("--gemm-mode", type=int, default=0, choices=(0, 1, 2),
                    help="arithmetic of the forward GEMMs for the HEADLINE line: 0 exact fp32 MFMA (default), "
                         "1 bf16x3 split, 2 bf16x2 split; a --full run reports modes 1 and 2 under extra")
    ap.add_argument("--train", choices=("nrms", "standard", "naml"), default=None,
                    help="time the data-parallel GRAD step instead (BASELINE configs[3]: impressions sharded over the "
                         "ranks, global in-batch InfoNCE through a differentiable all-gather, one flat RCCL gradient "
                         "all-reduce); prints its own JSON line")
    ap.add_argument("--overlap-buckets", action="store_true",
                    help="with --train: one gradient bucket per tower, all-reduced asynchronously as each completes during the "
                         "backward (default: one flat bucket after the backward)")
    ap.add_argument("--selftest-backend", choices=("gloo",), default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.gpus < 1:
        ap.error("--gpus must be >= 1")

    # ---- rank environment.  torch.distributed.run (the driver's N>1 launch) sets WORLD_SIZE; a bare
    # `python bench.py --gpus N` does not, and then THIS process is only the parent of the N ranks.
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch_ranks(args, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        # never print an n_gpus that differs from what was asked for
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; launch with --nproc-per-node {args.gpus} "
              f"(or without a launcher: bench.py starts the ranks itself)", file=sys.stderr)
        sys.exit(2)
    if args.selftest_backend and args.train:
        # the TRAINING line's launcher path on CPU: process group, rank count, weight broadcast, shard layout, embedding
        # all-gather, gradient-bucket all-reduce and the JSON line -- with a stand-in model (no hot-path work)
        torch.distributed.init_process_group(args.selftest_backend, rank=rank, world_size=world)
        ranks = count_ranks("cpu")
        out = train_scaling(args, torch.device("cpu"), rank, world, True)
        out["rccl_ranks"] = ranks
        out["metric"] = "launcher self-test of the training line (stub model, no hot-path work)"
        if rank == 0:
            print(json.dumps(out))
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
        return
    if args.selftest_backend:
        selftest_line(args, rank, world)
        return
    # XNRS_BENCH_FORCE_DIST=1 exercises the RCCL init / barrier / MAX-reduce path with a single rank
    dist_on = world > 1 or os.environ.get("XNRS_BENCH_FORCE_DIST") == "1"
    if local_rank >= torch.cuda.device_count():
        print(f"bench.py: rank {rank} needs GPU {local_rank} but {torch.cuda.device_count()} are visible", file=sys.stderr)
        sys.exit(2)
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    rccl_ranks = None
    if dist_on:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        torch.distributed.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
        rccl_ranks = count_ranks(device)
        if rccl_ranks != world:
            print(f"bench.py: RCCL all-reduce saw {rccl_ranks} ranks, expected {world}", file=sys.stderr)
            sys.exit(3)

    hip.set_gemm_mode(args.gemm_mode)  # explicit: the environment (XNRS_GEMM_MODE) never changes the headline
    mode_name, mode_products = GEMM_MODES[args.gemm_mode]
    if args.train:
        out = train_scaling(args, device, rank, world, dist_on)
        out["rccl_ranks"] = rccl_ranks
        if rank == 0:
            print(json.dumps(out))
        if dist_on:
            torch.distributed.barrier()
            torch.distributed.destroy_process_group()
        return
    w = WORKLOAD
    model, sd = build_model(w, device)
    hist, cand = make_inputs(w, device, seed=1000 + rank)  # each rank = its own shard of users

    last = {}

    def fn():
        last["scores"] = step(model, hist, cand)
        return last["scores"]

    with torch.no_grad():
        # warm-up outside the profiled region; with --full, profile ONLY the dominant kernel (stage 0) live
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        if args.full:
            hip.profile_enable(1)
        dt = timed(fn, args.steps, 0, dist_on)
        if args.full:
            prof = hip.profile_read()
            hip.profile_enable(0)
        scores = last["scores"]  # what the last timed step computed
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"scores": scores}, rank)

    n_gpus = world
    ms_per_step = dt / args.steps * 1e3
    value = n_gpus * w["B"] * args.steps / dt

    if rank == 0:
        out = {
            "metric": "impressions/sec (encode+score) on MIND-shaped batches",
            "value": value,
            "unit": "impressions/s",
            "n_gpus": n_gpus,
            "rccl_ranks": rccl_ranks,  # SUM all-reduce of ones over RCCL (null: single process, no process group)
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": mode_name,
            "data": "synthetic",
            "build_id": hip.build_id(),  # hash of the sources the measured binary was built from (= hip.tree_build_id())
            "build_is_tree": hip.build_id() == hip.tree_build_id(),
            "config": {"workload": "NRMS full user+news encode + 5-candidate dot scoring "
                                   "(BASELINE configs[2]; token shape of config/mind_small_NRMS.yml)",
                       "batch_impressions_per_gpu": w["B"], "history": w["H"], "candidates": w["C"],
                       "tokens": w["S"], "d_backbone": w["D"], "n_heads": w["h"], "emb_dim": w["E"],
                       "parallelism": f"impressions sharded by user over {n_gpus} GPU(s), no data-path collective",
                       "operation_order": ("every layer of the reference applied to every input; the attention out-projection is "
                                           "applied once per news behind the additive pooling instead of once per token (exact "
                                           "algebra, recomputed inside every timed step; extra.per_token_out_projection = the "
                                           "reference's order)" if fold_on() else "the reference's (XNRS_FOLD_OUT=0)")},
            # executed FLOPs (out-projection folded behind the pooling unless XNRS_FOLD_OUT=0); `reference_order_tflops` prices
            # the same impressions at the FLOPs of the reference's operation order -- it is NOT a utilisation figure
            "whole_path": {"alg_tflops": impression_flops(w, fold_on()) * value / n_gpus / 1e12,
                           "frac_fp32_mfma": impression_flops(w, fold_on()) * value / n_gpus / 1e12 / FP32_MFMA_PEAK_TFLOPS,
                           "out_projection": ("folded behind the pooling: fc1 on the attention rows with W1.Wo, one Wo product "
                                              "per news after the weighted sum (exact algebra, DESIGN.md section 4.6)"
                                              if fold_on() else "per token row (XNRS_FOLD_OUT=0)"),
                           "reference_order_tflops": impression_flops(w) * value / n_gpus / 1e12,
                           "alg_gbs": impression_bytes(w) * value / n_gpus / 1e9,
                           "frac_hbm": impression_bytes(w) * value / n_gpus / 1e9 / HBM_PEAK_GBS},
        }
        if args.full:
            out["roofline"] = qkv_roofline(prof, w, args.gemm_mode)
        if n_gpus == 1 and args.full:
            # the same step on a batch with EVERY history slot live: no all-zero news rows anywhere, so the dominant GEMM
            # multiplies random data throughout (the section-8d batch above has ~45 % all-zero rows, on which the chip
            # holds a higher clock); a few steps, same live hipEvent timing
            with torch.no_grad():
                hist_f, cand_f = make_inputs(w, device, seed=4000, full_history=True)
                fn_f = lambda: step(model, hist_f, cand_f)  # noqa: E731
                for _ in range(2):
                    fn_f()
                hip.profile_enable(1)
                dt_f = timed(fn_f, max(3, args.steps // 2), 0, False)
                pf = hip.profile_read()
                hip.profile_enable(0)
                del hist_f, cand_f
            f_ms, f_n, f_fl = pf["qkv_gemm"]
            ach_f = (f_fl / f_ms * 1e3 / 1e12) if f_ms > 0 else 0.0
            out["roofline"]["fully_live_random_batch"] = {
                "achieved": ach_f * mode_products, "frac": ach_f * mode_products / out["roofline"]["peak"],
                "avg_launch_ms": f_ms / max(f_n, 1), "launches_timed": f_n,
                "impressions_per_s": w["B"] * max(3, args.steps // 2) / dt_f,
                "note": "same step, every history slot live (no all-zero news rows)"}
            out["roofline_gather"] = gather_roofline(device)
        cpu_sample = None
        if n_gpus == 1 and args.full and not args.no_cpu_baseline:
            cb, ref = cpu_baseline(w, sd)
            out["cpu_baseline"] = cb
            # parity spot-check of the benchmarked model on the CPU sample (same weights)
            from oracle import xnrs_oracle as O  # noqa: F401
            b = synth.make_batch(77, 32, w["H"], w["C"], w["S"], w["D"], min_len=5)
            with torch.no_grad():
                got = model._forward(b["user_features"]["history"]["title_emb"], b["candidate_features"]["title_emb"])
            err = (got.cpu().double() - ref.double()).abs().max().item() / ref.abs().max().item()
            out["parity_max_rel_err_vs_cpu"] = err
            cpu_sample = (b, ref)
        else:
            out["cpu_baseline"] = None
        if n_gpus == 1 and args.full and not args.no_extra:
            with torch.no_grad():
                out["extra"] = {"news_encoder_only_1024": news_only_extra(device)}
                hip.profile_enable(hip.PROFILE_ALL)
                fn()
                torch.cuda.synchronize()
                st = hip.profile_read()
                hip.profile_enable(0)
                out["extra"]["stage_ms_per_step"] = {k: round(v[0], 3) for k, v in st.items()}
                out["extra"]["stage_tflops"] = {k: (v[2] / (v[0] * 1e-3) / 1e12 if v[0] > 0 else 0.0) for k, v in st.items()}
                out["extra"]["other_models_fwd_B512_H25"] = other_models_extra(device)
                out["extra"]["latency_one_impression"] = latency_extra(device)
                out["extra"]["id_path_B512"] = id_path_extra(device)
                out["extra"]["padding_free"] = padding_free_extra(model, hist, cand, args.steps, scores)
                if fold_on():
                    out["extra"]["per_token_out_projection"] = unfolded_extra(model, hist, cand, args.steps, scores)
                if args.gemm_mode == 0:
                    out["extra"]["gemm_modes"] = gemm_modes_extra(model, hist, cand, args.steps, scores, cpu_sample)
            out["extra"]["nrms_train_step_B64"] = train_step_extra(device, model_name="nrms")
            out["extra"]["standard_train_step_B64"] = train_step_extra(device, model_name="standard")
            out["extra"]["naml_train_step_B64"] = train_step_extra(device, model_name="naml")
            out["extra"]["ig_step"] = ig_step_extra(device)
            out["extra"]["eval_epoch"] = eval_epoch_extra(device)
            out["extra"]["store_file_to_hbm"] = store_upload_extra(device)
        assert torch.isfinite(scores).all()
        print(json.dumps(out))
    if dist_on:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
