#!/usr/bin/env python3
"""One timed run of phage_scoring's two parts on a FASTA (profiles/phage_scoring.md): palace_contig_features over every window
(device events around the enqueued launches), then the same windows with the model behind them.

    python tools/phage_scoring_time.py <assembly.fasta> <model state_dict> [records per window, default 1000] [records at most]

Prints one JSON line.  No comparison: the reference's script cannot run here."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    torch.zeros(1, device="cuda")
    from palace_amd import capi, scorer
    fasta, model = sys.argv[1:3]
    window = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
    limit = int(sys.argv[4]) if len(sys.argv) > 4 else 0
    text = open(fasta, "rb").read()
    n = len(text)
    t0 = time.perf_counter()
    state = scorer.load_state(model)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream), torch.no_grad(), capi.Ctx(0, stream=stream.cuda_stream) as ctx:
        weights = scorer.to_device(state, "cuda")
        stream.synchronize()
        t_model_load = time.perf_counter() - t0
        t0 = time.perf_counter()
        d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
        need = int(capi.lib().palace_fasta_index_scratch_bytes(n))
        d_scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        st = capi.fasta_index_at(ctx, d_text.data_ptr(), n, None, 0, d_scratch.data_ptr(), need)
        n_rec = int(st.n_records)
        d_recs = torch.empty((n_rec, 6), dtype=torch.int64, device="cuda")
        st = capi.fasta_index_at(ctx, d_text.data_ptr(), n, d_recs.data_ptr(), n_rec, d_scratch.data_ptr(), need)
        assert not st.error
        t_index = time.perf_counter() - t0
        bases = int(d_recs[:, 3].sum().item())
        n_use = min(n_rec, limit) if limit else n_rec
        feat = torch.empty((window, capi.CONTIG_FEATURES), dtype=torch.float32, device="cuda")
        fsum = torch.empty((window, capi.CONTIG_FSUMS), dtype=torch.float32, device="cuda")
        d_bad = torch.empty(1, dtype=torch.int64, device="cuda")
        need = int(capi.lib().palace_contig_features_scratch_bytes(n, window))
        d_scratch = torch.empty(need, dtype=torch.uint8, device="cuda")

        def features(r0):
            r1 = min(r0 + window, n_use)
            capi.contig_features_enqueue(ctx, d_text.data_ptr(), n, d_recs.data_ptr(), r0, r1, feat.data_ptr(), fsum.data_ptr(), None, d_bad.data_ptr(),
                                         d_scratch.data_ptr(), need)
            return r1 - r0

        out = {"fasta_bytes": n, "records": n_rec, "sequence_bytes": bases, "records_timed": n_use, "window": window,
               "model_load_s": round(t_model_load, 3), "upload_and_index_s": round(t_index, 3)}
        for label, with_model in (("features_warm_s", False), ("features_s", False), ("features_and_model_s", True)):
            beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            beg.record()
            for r0 in range(0, n_use, window):
                rows = features(r0)
                if with_model:
                    assert int(d_bad.item()) < 0
                    for m0 in range(0, rows, scorer.MODEL_BATCH):
                        scorer.forward(weights, feat[m0:min(m0 + scorer.MODEL_BATCH, rows)], fsum[m0:min(m0 + scorer.MODEL_BATCH, rows)])[0].cpu()
            end.record()
            end.synchronize()
            out[label] = round(beg.elapsed_time(end) / 1e3, 4)
        out["build"] = capi.lib().palace_version().decode()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
