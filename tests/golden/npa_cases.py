"""Generator parameters of the NPA fixtures (npa.json / npa.npz, written by make_golden_npa.py): the reference's NPA
(xnrs/models/full_models/npa.py:8-95) in eval mode and inside the MSE grad step (training.py:97-113,376-393).  Inputs and
weights regenerate from these seeds through xnrs_amd.synth on every machine; the fixtures hold outputs only."""
import numpy as np
import torch

# tiny: empty history slots (ragged histories), a repeated uid and uid 0 (the table has no padding row)
# shipped: config/mind_small_NPA.yml's shapes (50 x 768 tokens, A = 128, E = 256, du = 64, nh = 25, nc = 5) at a small B
CASES = {
    "tiny": dict(B=3, H=4, C=3, S=6, D=16, E=8, du=8, n_users=10, uids=[2, 0, 2], seed=900, min_len=1),
    "shipped": dict(B=2, H=25, C=5, S=50, D=768, E=256, du=64, n_users=40, uids=[7, 31], seed=910, min_len=5),
}
SCORERS = ("dot", "bilin", "fc")

# the state_dict contract of mind_small_NPA.yml at a small n_users; initial values under torch.manual_seed(INIT["seed"])
INIT = dict(config="mind_small_NPA", n_users=50, seed=0)

# tensors of more than SAMPLE_MIN elements are stored as a fixed SAMPLE_N-element sample (multiplicative hash walk)
SAMPLE_MIN, SAMPLE_N = 1024, 512


def sample(t):
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    if a.size <= SAMPLE_MIN:
        return a
    idx = (np.arange(SAMPLE_N, dtype=np.int64) * 2654435761 + 12345) % a.size
    return a.reshape(-1)[idx]


def model_cfg(c, scoring="dot"):
    """The flat YAML keys NPA and make_model read (npa.py:12-31, make_model.py:17-32)."""
    return dict(model="NPA", scoring=scoring, n_users=c["n_users"], user_emb_dim=c["du"], d_backbone=c["D"],
                title_emb_dim=c["E"], total_emb_dim=c["E"], p_dropout=0.0, bias=False, hist_len=c["H"], seq_len=c["S"],
                text_features=["title_emb"], catg_features=[], user_features=["user_index"], add_features=[])


def batch(c):
    """The reference's batch dict (dataset.py:67-158) with user_features.other.user_index:(B,1) int32."""
    from xnrs_amd import synth
    b = synth.make_batch(c["seed"], c["B"], c["H"], c["C"], c["S"], c["D"], min_len=c.get("min_len", 1))
    b["user_features"]["other"] = {"user_index": torch.tensor(c["uids"], dtype=torch.int32).reshape(-1, 1)}
    return b


def weight_seed(c):
    return c["seed"] + 1
