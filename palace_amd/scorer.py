"""The phage scorer of phage_scoring.py (GNN_Model.forward in eval mode) in plain torch, without torch_geometric.

The reference batches one bipartite graph per contig whose edges never change: feature node i (0 <= i < 4096) hangs on source
nodes i // 64 (forward edges) and i % 64 (backward edges).  So the two SAGE rounds are a broadcast, a mean over 64 rows and a few
GEMMs; what follows (the raw reshape, three Conv1d, two linear layers) is the reference's own torch.  The rules: DESIGN.md 8;
tests/scorer_cases.py holds the literal edge-list form this one is checked against."""
from __future__ import annotations

import torch
import torch.nn.functional as F

PNODES, FNODES, HIDDEN, GCN, CNN, TAPS, FC = 4096, 64, 3, 128, 64, 8, 100
FEATURES = PNODES * HIDDEN                          # PALACE_CONTIG_FEATURES
CONV_OUT = PNODES - 3 * (TAPS - 1)                  # 4075 positions behind three valid convolutions
D1_PIECES = 1600                                    # partial sums of d1: 260 800 = 1600 x 163
MODEL_BATCH = 64                                    # contigs per forward, as the reference's DataLoader

SHAPES = {
    "pnode_d.weight": (FEATURES, FEATURES), "pnode_d.bias": (FEATURES,),
    "fnode_d.weight": (FNODES * HIDDEN, FNODES), "fnode_d.bias": (FNODES * HIDDEN,),
    "convs_1.0.lin_l.weight": (GCN, HIDDEN), "convs_1.0.lin_l.bias": (GCN,), "convs_1.0.lin_r.weight": (GCN, HIDDEN),
    "convs_1.1.lin_l.weight": (GCN, GCN), "convs_1.1.lin_l.bias": (GCN,), "convs_1.1.lin_r.weight": (GCN, GCN),
    "convs_2.0.lin_l.weight": (GCN, GCN), "convs_2.0.lin_l.bias": (GCN,), "convs_2.0.lin_r.weight": (GCN, HIDDEN),
    "convs_2.1.lin_l.weight": (GCN, GCN), "convs_2.1.lin_l.bias": (GCN,), "convs_2.1.lin_r.weight": (GCN, GCN),
    "lns.0.weight": (GCN,), "lns.0.bias": (GCN,),
    "conv1.weight": (CNN, GCN, TAPS), "conv1.bias": (CNN,),
    "conv2.weight": (CNN, CNN, TAPS), "conv2.bias": (CNN,),
    "conv3.weight": (CNN, CNN, TAPS), "conv3.bias": (CNN,),
    "d1.weight": (FC, CONV_OUT * CNN), "d1.bias": (FC,),
    "d2.weight": (2, FC), "d2.bias": (2,),
}

CONVERSION = "torch.save(torch.load(p, weights_only=False).state_dict(), q)"


class ScorerError(ValueError):
    """a checkpoint this scorer does not take; the message names what is wrong"""


def check_state(state) -> None:
    """Every key of SHAPES with its shape, or ScorerError naming the first that is not.  (The reference loads with strict=False and
    would score with the random weights of whatever is missing.)"""
    if not isinstance(state, dict):
        raise ScorerError(f"model: not a state_dict but {type(state).__name__}")
    for key, shape in SHAPES.items():
        if key not in state:
            raise ScorerError(f"model: key {key} is missing")
        got = tuple(getattr(state[key], "shape", ()))
        if got != shape:
            raise ScorerError(f"model: key {key} has shape {got}, not {shape}")


def load_state(path: str) -> dict:
    """The state_dict checkpoint at path, on the CPU, checked."""
    state = None
    for mapped in (True, False):                    # mapped: the tensors are paged in as they are uploaded; older file formats cannot be
        try:
            state = torch.load(path, map_location="cpu", weights_only=True, mmap=mapped)
            break
        except OSError:
            raise
        except Exception as e:                      # at last: a pickled module, whose classes are torch_geometric's
            if not mapped:
                raise ScorerError(f"model: {path} is not a state_dict checkpoint ({type(e).__name__}). A whole-module pickle needs torch_geometric "
                                  f"to load; convert it once where torch_geometric is installed: {CONVERSION} (this conversion could not be tried "
                                  "here)") from e
    if hasattr(state, "state_dict"):
        raise ScorerError(f"model: {path} holds a module, not a state_dict; convert it: {CONVERSION}")
    check_state(state)
    return state


def to_device(state: dict, device, dtype=torch.float32) -> dict:
    return {k: state[k].to(device=device, dtype=dtype) for k in SHAPES}


def forward(w: dict, feat: torch.Tensor, fsum: torch.Tensor):
    """feat [B, 12288] with cell (d, a, b) at (a * 64 + b) * 3 + d, fsum [B, 64] -> (scores [B], logits [B, 2])"""
    b = feat.shape[0]
    x_p = F.linear(feat, w["pnode_d.weight"], w["pnode_d.bias"]).view(b, FNODES, FNODES, HIDDEN)      # node i = hi * 64 + lo at [hi, lo]
    x_f = F.linear(fsum, w["fnode_d.weight"], w["fnode_d.bias"]).view(b, FNODES, HIDDEN)
    for k in range(2):
        # forward edges: the one in-neighbour of feature node i is source node i // 64
        from_f = F.linear(x_f, w[f"convs_1.{k}.lin_l.weight"], w[f"convs_1.{k}.lin_l.bias"])
        x_p = F.relu(from_f[:, :, None, :] + F.linear(x_p, w[f"convs_1.{k}.lin_r.weight"]))
        # backward edges: source node j hears the 64 feature nodes with i % 64 = j, already updated
        x_f = F.relu(F.linear(x_p.mean(dim=1), w[f"convs_2.{k}.lin_l.weight"], w[f"convs_2.{k}.lin_l.bias"])
                     + F.linear(x_f, w[f"convs_2.{k}.lin_r.weight"]))
        if k == 0:
            x_p = F.layer_norm(x_p, (GCN,), w["lns.0.weight"], w["lns.0.bias"])
            x_f = F.layer_norm(x_f, (GCN,), w["lns.0.weight"], w["lns.0.bias"])
    x = x_p.reshape(b, GCN, PNODES)                 # the reference's raw reshape of (B * 4096, 128): not a transpose
    x = F.relu(F.conv1d(x, w["conv1.weight"], w["conv1.bias"]))
    x = F.relu(F.conv1d(x, w["conv2.weight"], w["conv2.bias"]))
    x = F.relu(F.conv1d(x, w["conv3.weight"], w["conv3.bias"]))
    # d1 is a sum of 260 800 terms: one float32 accumulation of that length is what carries the device's distance from float64
    # (profiles/phage_scoring.md), so it is summed in 1600 pieces of 163 terms (25 per conv channel) whose sums are then added
    parts = torch.einsum("bck,ock->boc", x.reshape(b, D1_PIECES, -1), w["d1.weight"].view(FC, D1_PIECES, -1))
    x = F.relu(parts.sum(dim=2) + w["d1.bias"])
    logits = F.linear(x, w["d2.weight"], w["d2.bias"])
    return F.softmax(logits, dim=1)[:, 1], logits
