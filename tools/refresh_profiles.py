#!/usr/bin/env python
"""Copy the judged summaries of one tools/gpu_profile.sh run (gpurun_out/prof_<tag>) into profiles/ (tracked).

    python tools/refresh_profiles.py <tag> [round-prefix, default r01]
"""
import csv
import datetime
import glob
import io
import json
import os
import shutil
import sys
from contextlib import redirect_stdout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import subprocess  # noqa: E402

import trace_summary  # noqa: E402

tag = sys.argv[1]
rnd = sys.argv[2] if len(sys.argv) > 2 else "r01"
gather_tag = sys.argv[3] if len(sys.argv) > 3 else None  # a tools/gpu_gather.sh run (gpurun_out/prof_<gather_tag>), optional
src = os.path.join(ROOT, "gpurun_out", f"prof_{tag}")
dst = os.path.join(ROOT, "profiles")

# 1. news-encoder pass: kernel trace + PMC passes (summary.txt without the torch helper kernels)
lines = [l for l in open(os.path.join(src, "summary.txt")) if "at::native" not in l and "rocclr" not in l]
with open(os.path.join(dst, f"{rnd}_rocprof_news_encoder_pass.txt"), "w") as f:
    f.write(f"# tools/gpu_profile.sh {tag}: rocprofv3 --kernel-trace --stats, then one --pmc pass per counter group (kernel trace only),\n"
            "# of `python3 tools/prof_news.py 1310 6 50 768 16` (six passes of the NRMS news encoder over one 65 500-row chunk), MI355X.\n")
    f.writelines(lines)

# 2. the bench command under the kernel tracer
buf = io.StringIO()
with redirect_stdout(buf):
    trace_summary.main(os.path.join(src, "bench_trace"))
with open(os.path.join(dst, f"{rnd}_bench_kernel_trace_summary.txt"), "w") as f:
    f.write("# rocprofv3 --kernel-trace --stats -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-extra   (MI355X)\n"
            "# per (kernel, grid) durations from the kernel trace; grid = threads.  The Q/K/V projection is gemm_f32_kernel<2,2,...> at grid 2359296\n"
            "# (9216 workgroups = 512 row tiles x 18 column tiles of one 65 500-row pass).\n")
    f.write(buf.getvalue())
stats = glob.glob(os.path.join(src, "bench_trace", "**", "*kernel_stats.csv"), recursive=True)[0]
rows = [r for r in csv.reader(open(stats))]
with open(os.path.join(dst, f"{rnd}_bench_kernel_stats.csv"), "w", newline="") as f:
    w = csv.writer(f)
    for r in rows:
        if r and (r[0] == "Name" or "xnrs::" in r[0]):
            w.writerow(r)
for l in open(os.path.join(src, "bench_trace.log")):
    if l.startswith('{"metric"'):
        json.dump(json.loads(l), open(os.path.join(dst, f"{rnd}_bench_under_rocprof.json"), "w"), indent=1)

# 3. traffic of the dominant kernel (FETCH_SIZE doubled: MI355X_MICROARCH.md, HBM)
def counter(passname, name):
    cc = glob.glob(os.path.join(src, f"pmc_{passname}", "**", "*counter_collection.csv"), recursive=True)[0]
    vals = [float(r["Counter_Value"]) for r in csv.DictReader(open(cc))
            if r["Counter_Name"] == name and "gemm_f32_kernel<2, 2," in r["Kernel_Name"] and r["Grid_Size"] == "2359296"]
    return sum(vals) / len(vals)

fetch, write = counter("fetch", "FETCH_SIZE"), counter("write", "WRITE_SIZE")
hit, req = counter("tcc", "TCC_HIT_sum"), counter("tcc", "TCC_REQ_sum")
rows_, D = 65500, 768
alg = rows_ * D * 4 + 3 * D * D * 4 + rows_ * 3 * D * 4
commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
dirty = bool(subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--", "xnrs_amd/csrc"], capture_output=True, text=True).stdout.strip())
# gather-only kernel (xnrs_gather_rows, 28 160 uniform ids into the 65 536-news table): counters of THIS round's
# tools/gpu_gather.sh run when its directory is given, else no figure at all (never a number copied from an older run)
gather_bytes, gather_note = None, "no tools/gpu_gather.sh run was passed to tools/refresh_profiles.py: no counter traffic for the gather kernel"
if gather_tag:
    gsrc = os.path.join(ROOT, "gpurun_out", f"prof_{gather_tag}")

    def gcounter(passname, name):
        cc = glob.glob(os.path.join(gsrc, f"uniform_pmc_{passname}", "**", "*counter_collection.csv"), recursive=True)
        vals = [float(r["Counter_Value"]) for r in csv.DictReader(open(cc[0])) if r["Counter_Name"] == name and "gather_rows_kernel<true>" in r["Kernel_Name"]
                and int(r["Grid_Size"]) > 1000000] if cc else []
        return sum(vals) / len(vals) if vals else None
    gf, gw = gcounter("fetch", "FETCH_SIZE"), gcounter("write", "WRITE_SIZE")
    if gf is not None and gw is not None:
        gather_bytes = int((2 * gf + gw) * 1024)
        gather_note = (f"gather_rows_kernel<true>, 28 160 uniform ids x 153 600-B news rows out of a 10-GB table: FETCH_SIZE {gf:.5g} KB (x2), "
                       f"WRITE_SIZE {gw:.5g} KB (tools/gpu_gather.sh {gather_tag}, this binary)")
json.dump({
    "commit": commit + ("+uncommitted csrc changes" if dirty else ""),
    "date": datetime.date.today().isoformat(),
    "method": "rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE in separate passes with --kernel-trace only; bytes = 2 x FETCH_SIZE + WRITE_SIZE (KB)",
    "gather_rows_hbm_bytes_per_launch": gather_bytes,
    "gather_note": gather_note,
    "qkv_launch": {"rows": rows_, "grid_threads": 2359296, "what": "one full 65 500-row pass (the last pass of a call is shorter)"},
    "source": f"rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate passes, --kernel-trace only), tools/gpu_profile.sh {tag}, MI355X; "
              f"see profiles/{rnd}_rocprof_news_encoder_pass.txt",
    "kernel": "gemm_f32_kernel<2,2,false,false,true,5,16,true,4,false,2> grid 2359296 (fused Q/K/V projection of one 65 500-row pass)",
    "FETCH_SIZE_KB_raw": fetch, "WRITE_SIZE_KB": write,
    "correction": "gfx950 FETCH_SIZE reports exactly 1/2 of the bytes of 16-B-per-lane coalesced loads (MI355X_MICROARCH.md, HBM): "
                  "reads doubled; WRITE_SIZE taken as is.  Cross-check: TCC_MISS_sum x 128 B = 2 x FETCH + WRITE within 2 %.",
    "qkv_gemm_hbm_bytes_per_launch": int((2 * fetch + write) * 1024),
    "algorithmic_bytes_per_launch": alg,
    "l2_hit_rate": hit / req,
    "note": "FETCH_SIZE counts L2-miss (fabric) requests and includes Infinity-Cache hits; A (201 MB) + W (7 MB) fit the 256 MB "
            "Infinity Cache, so the excess over the algorithmic 208 MB of reads is L2 re-fetch of operand tiles served on-die, not HBM "
            "traffic.  The grouped tile walk (3 groups of 6 column tiles) cut the raw FETCH_SIZE from 1.117e6 to 6.5e5 KB.",
}, open(os.path.join(dst, f"{rnd}_traffic.json"), "w"), indent=1)
print(open(os.path.join(dst, f"{rnd}_traffic.json")).read())
