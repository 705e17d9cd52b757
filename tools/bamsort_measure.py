"""profiles/bamsort.md: traced runs of `bamsort --bai` on the e2e leg's 1M-contig BAM with its records permuted (fixed seed), without and
with `--lz` in turns, and palace_sort_u64 alone at that many 53-bit keys.
    python tools/bamsort_measure.py [<log file> [<contigs>]]        (default tools/out/bamsort_measure.log, 1 000 000 contigs)"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from bench import e2e
from palace_amd import capi

log_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tools", "out", "bamsort_measure.log")
os.makedirs(os.path.dirname(os.path.abspath(log_path)), exist_ok=True)
out = open(log_path, "w")
def say(*a):
    print(*a); print(*a, file=out); out.flush()

work = "/tmp/bamsort_measure"
os.makedirs(work, exist_ok=True)
dev = torch.device("cuda" if torch.cuda.is_available() else "cpu")
n_contigs = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
n_pairs = int(5e8 * n_contigs / 1e6) // 150
gs = bench.make_graph_sample(torch, dev, n_contigs, n_pairs)
n = gs["n"]
rng = np.random.Generator(np.random.PCG64(12345))
p = rng.permutation(n)
pt = torch.as_tensor(p, device=dev)
so = gs["sa_off"].cpu().numpy().astype(np.int64)
has = (so[1:] - so[:-1]) > 0
gs["col"] = {k: v[pt].contiguous() for k, v in gs["col"].items()}
new_has = has[p]
rows = so[:-1][p][new_has]
gs["sa"] = gs["sa"][torch.as_tensor(rows, device=dev)].contiguous() if len(rows) else gs["sa"]
gs["sa_off"] = torch.as_tensor(np.concatenate([[0], np.cumsum(new_has)]).astype(np.int32), device=dev)
P = e2e.e2e_paths(work)
P["bam"] = os.path.join(work, "tmp.bam")
os.makedirs(P["cols"], exist_ok=True)
c = gs["col"]
for k in ("tid", "pos", "mtid", "mpos", "nm", "ref_len", "clip_e"):
    c[k].cpu().numpy().astype(np.int32).tofile(os.path.join(P["cols"], k + ".i32"))
gs["sa_off"].cpu().numpy().astype(np.int32).tofile(os.path.join(P["cols"], "sa_off.i32"))
gs["sa"][: max(1, gs["n_sa"])].cpu().numpy().astype(np.int32).tofile(os.path.join(P["cols"], "sa.i32"))
c["flag"].cpu().numpy().view(np.uint16).tofile(os.path.join(P["cols"], "flag.u16"))
c["mapq"].cpu().numpy().tofile(os.path.join(P["cols"], "mapq.u8"))
c["qkey"].cpu().numpy().view(np.uint64).tofile(os.path.join(P["cols"], "qkey.u64"))
with open(os.path.join(P["cols"], "targets.tsv"), "w") as f:
    f.write("".join(f"{nm}\t{l}\n" for nm, l in zip(gs["names"], gs["lens"].tolist())))
subprocess.run([os.path.join(ROOT, "palace_amd", "bin", "synthbam"), P["cols"], P["bam"], "16", "1"], check=True)
say(f"input: {n} records, {n_contigs} targets, {os.path.getsize(P['bam'])} B (zlib level 1, records permuted with seed 12345)")
sorted_bam, lz_bam = os.path.join(work, "first.bam"), os.path.join(work, "first_lz.bam")
# the two coders in turns in one call: the unflagged run is the yardstick of the --lz run next to it.  The first run also pays the
# code objects' load; every run is printed
for rep in range(3):
    for flags, dst in (([], sorted_bam), (["--lz"], lz_bam)):
        t0 = time.perf_counter()
        r = subprocess.run([os.path.join(ROOT, "palace_amd", "bin", "bamsort"), "-@", "16"] + flags + [P["bam"], "-O", "BAM", "-o", dst, "--bai"],
                           env=dict(os.environ, PALACE_TRACE="1"), stderr=subprocess.PIPE, timeout=300)
        say(f"run {rep}{' --lz' if flags else ''}: exit {r.returncode}, wall {time.perf_counter() - t0:.3f} s, output {os.path.getsize(dst) if r.returncode == 0 else 0} B")
        say(r.stderr.decode())
        if r.returncode:
            sys.exit(1)
r = subprocess.run([os.path.join(ROOT, "palace_amd", "bin", "bamsort"), "--index", lz_bam, os.path.join(work, "again_lz.bai")], stderr=subprocess.PIPE, timeout=300)
say(f"--lz: --index exit {r.returncode}; same bytes as --bai: {open(os.path.join(work, 'again_lz.bai'), 'rb').read() == open(lz_bam + '.bai', 'rb').read()}")
say(f"output: {os.path.getsize(sorted_bam)} B, .bai {os.path.getsize(sorted_bam + '.bai')} B")
r = subprocess.run([os.path.join(ROOT, "palace_amd", "bin", "bamsort"), "--index", sorted_bam, os.path.join(work, "again.bai")], stderr=subprocess.PIPE, timeout=300)
say(f"--index exit {r.returncode}; same bytes as --bai: {open(os.path.join(work, 'again.bai'), 'rb').read() == open(sorted_bam + '.bai', 'rb').read()}")
r = subprocess.run([os.path.join(ROOT, "palace_amd", "bin", "bamsort"), "-o", os.path.join(work, "again.bam"), sorted_bam], stderr=subprocess.PIPE, timeout=300)
say(f"sorting the output again: exit {r.returncode}; same file: {open(os.path.join(work, 'again.bam'), 'rb').read() == open(sorted_bam, 'rb').read()}")
r = subprocess.run([os.path.join(ROOT, "palace_amd", "bin", "bamsort"), "-o", os.path.join(work, "again.bam"), lz_bam], stderr=subprocess.PIPE, timeout=300)
say(f"sorting the --lz output without the flag: exit {r.returncode}; the unflagged run's file (so the same stream): "
    f"{open(os.path.join(work, 'again.bam'), 'rb').read() == open(sorted_bam, 'rb').read()}")

# the sort alone: n keys of 53 bits, as the tool's (20 bits of refID + 33)
keys = rng.integers(0, 1 << 53, n, dtype=np.uint64)
want = np.argsort(keys, kind="stable")
with capi.Ctx() as ctx:
    nscr = int(capi.lib().palace_sort_u64_scratch_bytes(n))
    d_src, d_key, d_perm, d_scr = ctx.upload(keys), ctx.empty(n, np.uint64), ctx.empty(n, np.uint32), capi.DevBuf(ctx, nscr)
    ms = []
    for rep in range(12):
        capi._check(capi.lib().palace_d2d(ctx.h, d_key.ptr, d_src.ptr, n * 8), "d2d")
        capi._check(capi.lib().palace_sync(ctx.h), "sync")
        t0 = time.perf_counter()
        capi._check(capi.lib().palace_sort_u64(ctx.h, d_key.ptr, d_perm.ptr, n, 53, d_scr.ptr, nscr), "sort")
        capi._check(capi.lib().palace_sync(ctx.h), "sync")
        ms.append((time.perf_counter() - t0) * 1e3)
    ok = np.array_equal(d_perm.to_host(), want.astype(np.uint32))
    say(f"palace_sort_u64 alone, {n} keys, key_bits 53 (7 passes), host clock around call + sync, 12 runs: first {ms[0]:.3f} ms, "
        f"then min {min(ms[2:]):.3f} median {sorted(ms[2:])[len(ms[2:]) // 2]:.3f} max {max(ms[2:]):.3f} ms; result == numpy stable argsort: {ok}")
out.close()
