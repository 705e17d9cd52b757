"""The reference's GNN_Model.forward written out literally for the scorer tests: the edge list of make_edge(), the batching
offsets of its BipartiteData, SAGEConv's mean aggregation as a scatter-mean by index_add_ -- no torch_geometric.  And a seeded
checkpoint at the model's real shapes.  Not a test module."""
import numpy as np
import torch
import torch.nn.functional as F

from palace_amd import scorer


def make_edge() -> np.ndarray:
    edge = []
    for i in range(4096):
        edge.append([i // 64, i])
        edge.append([i % 64, i])
    return np.array(edge).T


def seeded_state(seed: int, dtype=torch.float32, d1_scale: float = 1.0, d2_scale: float = 1.0) -> dict:
    """torch's default initialisation in kind (uniform within 1 / sqrt(fan in)), LayerNorm off its identity so that it shows;
    d1 and d2 scaled so that the scores of different contigs lie apart"""
    g = torch.Generator().manual_seed(seed)
    state = {}
    for key, shape in scorer.SHAPES.items():
        layer = key.rsplit(".", 1)[0]
        fan_in = int(np.prod(scorer.SHAPES[layer + ".weight"][1:])) if len(scorer.SHAPES[layer + ".weight"]) > 1 else 1
        t = (torch.rand(shape, generator=g, dtype=torch.float32) * 2 - 1) / fan_in ** 0.5
        if key == "lns.0.weight":
            t = 1 + 0.25 * t
        if key == "lns.0.bias":
            t = 0.25 * t
        if layer == "d1":
            t = t * d1_scale
        if layer == "d2":
            t = t * d2_scale
        state[key] = t.to(dtype)
    return state


def _sage(x_src, x_dst, edge_index, lin_l_w, lin_l_b, lin_r_w):
    """SAGEConv((src, dst), out) with mean aggregation: lin_l(mean of the in-neighbours) + lin_r(x_dst)"""
    src, dst = edge_index[0], edge_index[1]
    total = torch.zeros(x_dst.shape[0], x_src.shape[1], dtype=x_src.dtype).index_add_(0, dst, x_src[src])
    count = torch.zeros(x_dst.shape[0], dtype=x_src.dtype).index_add_(0, dst, torch.ones(dst.shape[0], dtype=x_src.dtype))
    mean = total / count.clamp(min=1)[:, None]
    return F.linear(mean, lin_l_w, lin_l_b) + F.linear(x_dst, lin_r_w)


def literal_forward(w: dict, feat: torch.Tensor, fsum: torch.Tensor):
    """(scores, logits) on the CPU in the dtype of the inputs"""
    n = feat.shape[0]
    template = torch.tensor(make_edge(), dtype=torch.long)
    edge_index = torch.cat([template + torch.tensor([[64 * g], [4096 * g]]) for g in range(n)], dim=1)     # BipartiteData.__inc__
    forward = edge_index[:, ::2]
    backward = edge_index[[1, 0], :][:, 1::2]
    x_p = torch.reshape(feat, (-1, 4096 * 3))
    x_p = F.linear(x_p, w["pnode_d.weight"], w["pnode_d.bias"])
    x_p = torch.reshape(x_p, (-1, 3))
    x_f = torch.reshape(fsum, (-1, 64))
    x_f = F.linear(x_f, w["fnode_d.weight"], w["fnode_d.bias"])
    x_f = torch.reshape(x_f, (-1, 3))
    for i in range(2):
        x_p = F.relu(_sage(x_f, x_p, forward, w[f"convs_1.{i}.lin_l.weight"], w[f"convs_1.{i}.lin_l.bias"], w[f"convs_1.{i}.lin_r.weight"]))
        x_f = F.relu(_sage(x_p, x_f, backward, w[f"convs_2.{i}.lin_l.weight"], w[f"convs_2.{i}.lin_l.bias"], w[f"convs_2.{i}.lin_r.weight"]))
        if i < 1:
            x_p = F.layer_norm(x_p, (128,), w["lns.0.weight"], w["lns.0.bias"])
            x_f = F.layer_norm(x_f, (128,), w["lns.0.weight"], w["lns.0.bias"])
    x = torch.reshape(x_p, (-1, 128, 4096))
    x = F.relu(F.conv1d(x, w["conv1.weight"], w["conv1.bias"]))
    x = F.relu(F.conv1d(x, w["conv2.weight"], w["conv2.bias"]))
    x = F.relu(F.conv1d(x, w["conv3.weight"], w["conv3.bias"]))
    x = x.flatten(start_dim=1)
    x = F.relu(F.linear(x, w["d1.weight"], w["d1.bias"]))
    logits = F.linear(x, w["d2.weight"], w["d2.bias"])
    return F.softmax(logits, dim=1)[:, 1], logits


# the scorer tests' checkpoint and contigs: one seed, d1 and d2 scaled until the float64 scores span 0.1 (test_gpu_scorer asserts it)
TEST_SEED, D1_SCALE, D2_SCALE = 7, 8.0, 8.0
CONTIG_LENGTHS = (300, 1200, 4100, 9000, 25000, 60000)


def scorer_contigs():
    """(name, sequence) pairs of different composition, so that their features and scores differ"""
    rng = np.random.default_rng(77)
    out = []
    for k, n in enumerate(CONTIG_LENGTHS):
        p = rng.dirichlet(np.full(4, 1.5))
        seq = np.frombuffer(b"ACGT", np.uint8)[rng.choice(4, size=n, p=p)].copy()
        seq[rng.integers(0, n, size=n // 100)] = ord("N")
        out.append((b"contig_%d" % k, seq.tobytes()))
    return out


_SHARED = {}


def checkpoint():
    """the tests' float32 state_dict, made once per process"""
    if "state" not in _SHARED:
        _SHARED["state"] = seeded_state(TEST_SEED, torch.float32, D1_SCALE, D2_SCALE)
    return _SHARED["state"]


def reference():
    """(features [6, 12288] and row sums [6, 64] of the golden-pinned restatement as float32 tensors, then the literal form's
    float64 scores and logits over them) -- computed once per process and left as it is"""
    if "reference" not in _SHARED:
        from tests import contig_feature_cases as cc
        rows = [cc.model_features(seq) for _, seq in scorer_contigs()]
        feat = torch.tensor(np.stack([r[0] for r in rows]))
        fsum = torch.tensor(np.stack([r[1] for r in rows]))
        w64 = {k: v.double() for k, v in checkpoint().items()}
        with torch.no_grad():
            scores, logits = literal_forward(w64, feat.double(), fsum.double())
        _SHARED["reference"] = (feat, fsum, scores.numpy(), logits.numpy())
    return _SHARED["reference"]


# Measured on the CPU with this checkpoint and these contigs (profiles/phage_scoring.md): the literal form in float32 is
# 1.16e-7 (scores) and 3.89e-7 (logits) away from the literal form in float64.  The device may be four times as far.
TOL_SCORES, TOL_LOGITS = 4 * 1.16e-7, 4 * 3.89e-7
