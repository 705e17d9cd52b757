"""palace_amd.scorer.forward (reshapes, a mean over 64 rows, GEMMs) against the reference's forward written out literally with its
edge list (tests/scorer_cases.py), both on the CPU in float64 with seeded weights at the model's real shapes; and the checkpoint
check.  The bound 1e-9: float64 sums of at most 260 800 terms of order 1 in two orders differ by far less."""
import numpy as np
import pytest
import torch

from palace_amd import scorer
from tests import contig_feature_cases as cc
from tests import scorer_cases as sc


@pytest.fixture(scope="module")
def weights():
    return sc.seeded_state(sc.TEST_SEED, torch.float64, sc.D1_SCALE, sc.D2_SCALE)


def test_structured_form_equals_the_literal_form(weights):
    rows = [cc.model_features(seq) for _, seq in sc.scorer_contigs()[:3]]
    feat = torch.tensor(np.stack([r[0] for r in rows])).double()
    fsum = torch.tensor(np.stack([r[1] for r in rows])).double()
    with torch.no_grad():
        want_scores, want_logits = sc.literal_forward(weights, feat, fsum)
        got_scores, got_logits = scorer.forward(weights, feat, fsum)
    assert got_scores.shape == (3,) and got_logits.shape == (3, 2) and got_scores.dtype == torch.float64
    d_scores, d_logits = float((got_scores - want_scores).abs().max()), float((got_logits - want_logits).abs().max())
    print("structured against literal, float64: scores", d_scores, "logits", d_logits)
    assert d_scores <= 1e-9 and d_logits <= 1e-9
    assert float(want_scores.max() - want_scores.min()) > 1e-3           # the three contigs do not score alike


def test_the_edge_list_is_the_fixed_bipartite_graph():
    edge = sc.make_edge()
    assert edge.shape == (2, 8192)
    assert (edge[:, ::2] == np.stack([np.arange(4096) // 64, np.arange(4096)])).all()
    assert (edge[:, 1::2] == np.stack([np.arange(4096) % 64, np.arange(4096)])).all()


def meta_state():
    return {k: torch.empty(shape, device="meta") for k, shape in scorer.SHAPES.items()}


def test_a_complete_state_passes():
    scorer.check_state(meta_state())
    assert scorer.SHAPES["d1.weight"] == (100, 260800) and len(scorer.SHAPES) == 28


@pytest.mark.parametrize("key", ["pnode_d.weight", "convs_2.0.lin_r.weight", "lns.0.bias", "d2.bias"])
def test_a_missing_key_is_refused_by_name(key):
    state = meta_state()
    del state[key]
    with pytest.raises(scorer.ScorerError, match="key " + key.replace(".", r"\.") + " is missing"):
        scorer.check_state(state)


@pytest.mark.parametrize("key, shape", [("convs_1.0.lin_r.weight", (128, 128)), ("d1.weight", (100, 4075)), ("conv1.bias", (128,))])
def test_a_wrong_shape_is_refused_by_name(key, shape):
    state = meta_state()
    state[key] = torch.empty(shape, device="meta")
    with pytest.raises(scorer.ScorerError, match="key " + key.replace(".", r"\.") + " has shape"):
        scorer.check_state(state)


def test_a_pickled_module_is_refused_with_the_conversion(tmp_path):
    path = tmp_path / "whole_module.pt"
    torch.save(torch.nn.Linear(2, 2), str(path))
    with pytest.raises(scorer.ScorerError, match="state_dict"):
        scorer.load_state(str(path))
    with pytest.raises(scorer.ScorerError) as e:
        scorer.load_state(str(path))
    assert scorer.CONVERSION in str(e.value)
