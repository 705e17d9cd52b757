#!/usr/bin/env python3
"""Kernel times of the paths -> FASTA chain on the files of tools/path_fasta_synth.py (profiles/path_fasta.md; one MI355X).

    python tools/path_fasta_time.py <dir with assembly.fasta and paths.txt> [--window BYTES] [--reps N]

HIP-event times (palace_timer_begin / _end on the context's stream) of palace_fasta_index, palace_path_resolve,
palace_path_fasta_lengths and of palace_path_fasta_write per window, through the ctypes view of the library.  The executable
cannot be profiled from outside: it leaves through _exit once its outputs are complete (host/fast_exit.hpp), so a profiler
attached to it never writes its files.  The paths file is split here in Python (clean tokens, TAB separated, as the generator writes)."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from palace_amd import capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--window", type=int, default=256 << 20)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    fasta = np.fromfile(os.path.join(a.dir, "assembly.fasta"), np.uint8)
    lines = [l.split(b"\t") for l in open(os.path.join(a.dir, "paths.txt"), "rb").read().split(b"\n") if l]
    lib = capi.lib()
    with capi.Ctx(0) as ctx:
        d_text = ctx.upload(fasta)
        d_scratch = capi.DevBuf(ctx, int(lib.palace_fasta_index_scratch_bytes(len(fasta))))
        st = capi.FastaStatus()
        capi._check(lib.palace_fasta_index(ctx.h, d_text.ptr, len(fasta), None, 0, d_scratch.ptr, d_scratch.nbytes, C.byref(st)), "palace_fasta_index")
        n_rec = int(st.n_records)
        d_recs = ctx.empty((n_rec,), capi.FASTA_REC_DTYPE)
        for _ in range(a.reps):
            ctx.timer_begin()
            capi._check(lib.palace_fasta_index(ctx.h, d_text.ptr, len(fasta), d_recs.ptr, n_rec, d_scratch.ptr, d_scratch.nbytes, C.byref(st)), "palace_fasta_index")
            ms = ctx.timer_end()
            print(f"palace_fasta_index: {len(fasta)} bytes, {n_rec} records, error {st.error}: {ms:.3f} ms = {len(fasta) / ms / 1e6:.1f} GB/s of text")
        names = C.c_void_p()
        ctx.timer_begin()
        capi._check(lib.palace_fasta_names_create(ctx.h, d_text.ptr, d_recs.ptr, n_rec, None, C.byref(names)), "palace_fasta_names_create")
        print(f"palace_fasta_names_create: {ctx.timer_end():.3f} ms")
        tokens = [t for l in lines for t in l]
        tok_off = np.zeros(len(tokens) + 1, np.int64)
        np.cumsum([len(t) for t in tokens], out=tok_off[1:])
        path_off = np.zeros(len(lines) + 1, np.int64)
        np.cumsum([len(l) for l in lines], out=path_off[1:])
        d_tok, d_tok_off, d_path_off = ctx.upload(np.frombuffer(b"".join(tokens), np.uint8)), ctx.upload(tok_off), ctx.upload(path_off)
        d_code, d_cum, d_len = ctx.empty((len(tokens),), np.int32), ctx.empty((len(tokens) + 1,), np.int64), ctx.empty((len(lines),), np.int64)
        ctx.timer_begin()
        capi._check(lib.palace_path_resolve(ctx.h, names, d_tok.ptr, d_tok_off.ptr, len(tokens), d_code.ptr), "palace_path_resolve")
        print(f"palace_path_resolve: {len(tokens)} tokens: {ctx.timer_end():.3f} ms")
        ctx.timer_begin()
        capi._check(lib.palace_path_fasta_lengths(ctx.h, d_recs.ptr, d_code.ptr, len(tokens), d_path_off.ptr, len(lines), d_cum.ptr, d_len.ptr),
                    "palace_path_fasta_lengths")
        print(f"palace_path_fasta_lengths: {len(lines)} paths: {ctx.timer_end():.3f} ms")
        assert (d_code.to_host() >= 0).all()
        lens = d_len.to_host()
        headers = [b"res_%d_%d" % (i + 1, int(l)) for i, l in enumerate(lens)]
        hdr_off = np.zeros(len(lines) + 1, np.int64)
        np.cumsum([len(h) for h in headers], out=hdr_off[1:])
        path_out = np.zeros(len(lines) + 1, np.int64)
        path_out[1:] = np.cumsum(np.diff(hdr_off) + lens + 3)
        total = int(path_out[-1])
        d_hdr, d_hdr_off, d_path_out = ctx.upload(np.frombuffer(b"".join(headers), np.uint8)), ctx.upload(hdr_off), ctx.upload(path_out)
        d_out = capi.DevBuf(ctx, min(a.window, total))
        for rep in range(a.reps):
            all_ms = 0.0
            for lo in range(0, total, a.window):
                hi = min(total, lo + a.window)
                ctx.timer_begin()
                capi._check(lib.palace_path_fasta_write(ctx.h, d_text.ptr, d_recs.ptr, d_code.ptr, d_cum.ptr, d_path_off.ptr, len(lines), d_hdr.ptr, d_hdr_off.ptr,
                                                        d_path_out.ptr, lo, hi, d_out.ptr), "palace_path_fasta_write")
                ms = ctx.timer_end()
                all_ms += ms
                if rep == a.reps - 1:
                    print(f"palace_path_fasta_write [{lo}, {hi}): {ms:.3f} ms = {(hi - lo) / ms / 1e6:.1f} GB/s written")
            print(f"palace_path_fasta_write, the whole text, {total} bytes: {all_ms:.3f} ms = {total / all_ms / 1e6:.1f} GB/s written")
        capi._check(lib.palace_fasta_names_destroy(ctx.h, names), "palace_fasta_names_destroy")


if __name__ == "__main__":
    main()
