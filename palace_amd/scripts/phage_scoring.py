#!/usr/bin/env python3
"""Score every contig of a FASTA with the phage model: `name<TAB>score` lines.

Counterpart of the reference's share/palace/scripts/phage_scoring.py (call site palace:461-470), the same command line
    phage_scoring.py <fasta> <out> <reverse> <threads> <model_path> [batch_size]
where <reverse> and <threads> are accepted and ignored and batch_size (1000) is the number of records per feature window.  The
features are palace_contig_features's (the FASTA indexed and the k-mer pairs counted on the GPU; the rules: DESIGN.md 8), the model
is palace_amd/scorer.py in float32 on the same stream, 64 contigs at a time.  There is no CPU path: without a device the step
fails.  The text, its records and one window have to fit the device.
Deviations, declared: a digit in a sequence is a fault (the reference counts 0-3 as bases and raises on 4-9); the model file must
be a state_dict with every key at its shape (the reference loads with strict=False and would score with random weights).
Parity status: the feature rules are PINNED (tests/golden/contig_features_cases.npz holds what the reference's compiled encoder
returned); the model is UNPINNED -- torch_geometric and the model file are absent, it rests on two restatements that agree.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FAULTS = {1: "text before the first '>'", 2: "a header line without a name",
          3: "a sequence line behind a line of another length than the record's first (only a record's last line may be shorter)",
          4: "a sequence line behind a blank line of its record", 5: "a sequence byte outside 0x21-0x7E"}


class Failure(Exception):
    pass


def score(fasta: str, model_path: str, window: int):
    """the output's lines"""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise Failure("no ROCm device: there is no CPU path")
    from palace_amd import capi, scorer
    torch.zeros(1, device="cuda")                   # torch's HIP runtime is the one the process uses; the library comes second
    try:
        state = scorer.load_state(model_path)
    except scorer.ScorerError as e:
        raise Failure(str(e))
    except OSError as e:
        raise Failure(f"model: {e}")
    with open(fasta, "rb") as f:
        text = f.read()
    n = len(text)
    if n == 0:
        return []
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream), torch.no_grad(), capi.Ctx(torch.cuda.current_device(), stream=stream.cuda_stream) as ctx:
        d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
        need = max(int(capi.lib().palace_fasta_index_scratch_bytes(n)), 16)
        d_scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        st = capi.fasta_index_at(ctx, d_text.data_ptr(), n, None, 0, d_scratch.data_ptr(), need)
        if not st.error:
            n_rec = int(st.n_records)
            d_recs = torch.empty((max(n_rec, 1), 6), dtype=torch.int64, device="cuda")
            st = capi.fasta_index_at(ctx, d_text.data_ptr(), n, d_recs.data_ptr(), n_rec, d_scratch.data_ptr(), need)
        if st.error:
            raise Failure(f"{fasta}: line {int(st.bad_line)}: {FAULTS.get(int(st.error), 'malformed')}")
        del d_scratch
        if n_rec == 0:
            return []
        weights = scorer.to_device(state, "cuda")
        recs = d_recs.cpu().numpy()
        names = [text[int(o):int(o) + int(l)].decode("ascii", "replace") for o, l in zip(recs[:n_rec, 0], recs[:n_rec, 1])]
        window = max(1, min(window, n_rec))
        feat = torch.empty((window, capi.CONTIG_FEATURES), dtype=torch.float32, device="cuda")
        fsum = torch.empty((window, capi.CONTIG_FSUMS), dtype=torch.float32, device="cuda")
        d_bad = torch.empty(1, dtype=torch.int64, device="cuda")
        need = max(int(capi.lib().palace_contig_features_scratch_bytes(n, window)), 16)
        d_scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        scores = []
        for r0 in range(0, n_rec, window):
            r1 = min(r0 + window, n_rec)
            capi.contig_features_enqueue(ctx, d_text.data_ptr(), n, d_recs.data_ptr(), r0, r1, feat.data_ptr(), fsum.data_ptr(), None,
                                         d_bad.data_ptr(), d_scratch.data_ptr(), need)
            bad = int(d_bad.item())
            if bad >= 0:
                line = text.count(b"\n", 0, bad) + 1
                raise Failure(f"{fasta}: line {line}: digit in sequence")
            for m0 in range(0, r1 - r0, scorer.MODEL_BATCH):
                m1 = min(m0 + scorer.MODEL_BATCH, r1 - r0)
                scores.append(scorer.forward(weights, feat[m0:m1], fsum[m0:m1])[0].cpu().numpy())
        stream.synchronize()
    return [f"{name}\t{format(np.float32(p), '')}" for name, p in zip(names, np.concatenate(scores))]


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) < 5:
        print("Usage: phage_scoring.py <fasta> <out> <reverse> <threads> <model_path> [batch_size]", file=sys.stderr)
        return 1
    fasta, out, _, _, model_path = argv[:5]
    tmp = out + ".tmp"
    try:
        window = int(argv[5]) if len(argv) > 5 else 1000
        if window < 1:
            raise Failure("batch_size must be at least 1")
        lines = score(fasta, model_path, window)     # nothing is written before every window's digit report is in
        with open(tmp, "w") as f:
            f.write("\n".join(lines))                # no LF behind the last line, as the reference writes it
        os.replace(tmp, out)
    except (Failure, OSError, ValueError) as e:
        if os.path.exists(tmp):
            os.remove(tmp)
        print(f"phage_scoring: {e}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
