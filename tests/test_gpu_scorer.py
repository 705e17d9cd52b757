"""The scorer on the ROCm device: features from palace_contig_features, palace_amd.scorer.forward in float32, against the
reference's forward written out literally (tests/scorer_cases.py) on the CPU in float64 over the restatement's features.
Tolerance: four times what the literal form in float32 on the CPU is away from the same float64 values
(profiles/phage_scoring.md) -- hipBLASLt and MIOpen sum in another order and at another blocking."""
import numpy as np
import pytest
import torch

from palace_amd import capi, scorer
from tests import contig_feature_cases as cc
from tests import scorer_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device_out(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("scorer") / "model.pt")
    torch.save(sc.checkpoint(), path)
    weights = scorer.to_device(scorer.load_state(path), "cuda")
    text, _ = cc.fasta(sc.scorer_contigs())
    with capi.Ctx(0) as ctx:
        _, _, feat, fsum, _, bad = capi.contig_features(ctx, text)
    assert bad == -1
    with torch.no_grad():
        scores, logits = scorer.forward(weights, torch.tensor(feat).cuda(), torch.tensor(fsum).cuda())
    assert scores.dtype == torch.float32 and scores.is_cuda
    return feat, fsum, scores.cpu().numpy().astype(np.float64), logits.cpu().numpy().astype(np.float64)


def test_contigs_and_reference_can_tell_scores_apart():
    lengths = [len(s) for _, s in sc.scorer_contigs()]
    assert len(lengths) == 6 and min(lengths) == 300 and max(lengths) == 60000
    _, _, scores, _ = sc.reference()
    assert scores.max() - scores.min() >= 0.1, scores


def test_device_features_are_the_restatements(device_out):
    feat, fsum, _, _ = sc.reference()
    assert device_out[0].tobytes() == feat.numpy().tobytes() and device_out[1].tobytes() == fsum.numpy().tobytes()


def test_device_scores_against_the_literal_form(device_out):
    _, _, want_scores, want_logits = sc.reference()
    _, _, scores, logits = device_out
    d_scores, d_logits = np.abs(scores - want_scores).max(), np.abs(logits - want_logits).max()
    print("device float32 against literal float64: scores", d_scores, "logits", d_logits, "allowed", sc.TOL_SCORES, sc.TOL_LOGITS)
    assert d_scores <= sc.TOL_SCORES and d_logits <= sc.TOL_LOGITS


def test_a_permuted_distance_axis_is_seen(device_out):
    """d rotated in the feature layout on the reference side: the device's scores must then be off by more than the tolerance"""
    feat, fsum, _, _ = sc.reference()
    moved = feat.view(-1, 4096, 3)[:, :, [1, 2, 0]].reshape(-1, 12288)
    w64 = {k: v.double() for k, v in sc.checkpoint().items()}
    with torch.no_grad():
        scores, logits = sc.literal_forward(w64, moved.double(), fsum.double())
    _, _, got_scores, got_logits = device_out
    d_scores, d_logits = np.abs(got_scores - scores.numpy()).max(), np.abs(got_logits - logits.numpy()).max()
    print("against the permuted reference: scores", d_scores, "logits", d_logits)
    assert d_scores > 100 * sc.TOL_SCORES and d_logits > 100 * sc.TOL_LOGITS
