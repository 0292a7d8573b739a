"""Generator parameters of the CAUM fixtures (caum.json / caum.npz, written by make_golden_caum.py): the reference's CAUM
(xnrs/models/full_models/caum.py:11-172) with its CAUMScoring scorer in eval mode and inside the MSE grad step
(training.py:97-113,376-393).  Inputs and weights regenerate from these seeds through xnrs_amd.synth on every machine; the
fixtures hold outputs only.

Dropout.  The grad step runs with every module in eval mode (the news encoder's attention-probability dropout draws from
torch's generator and cannot be matched); p_dropout is 0 except in `dropmask`, where user_encoder.dropout1 / dropout2 /
dropout3 are replaced by FixedMaskDropout modules IN TRAIN MODE -- a seed-generated mask / (1 - p) -- on both sides."""
import numpy as np
import torch
import torch.nn as nn

# the smallest shapes at which each piece can still go wrong (B impressions, H history slots, C candidates, S tokens of
# D columns, E = Et + Ec [+ Ec with the sub-category]); the attention runs along L = B * C with H as its batch
_TINY = dict(B=3, H=6, C=4, S=5, D=32, Et=24, Ec=8, heads=4, bias=True, subcat=False, p=0.0, min_len=1)
CASES = {
    "tiny": dict(_TINY, seed=1300),                                   # L = 12; ragged histories: all-masked trailing slots
    "odd_dk": dict(_TINY, Et=26, heads=2, bias=False, seed=1310),     # E = 34, d_k = 17
    "subcat": dict(_TINY, subcat=True, bias=False, seed=1320),        # E = 24 + 2 * 8 = 40, d_k = 10
    "h1": dict(_TINY, H=1, seed=1330),                                # left = middle = right slot
    "h2": dict(_TINY, H=2, bias=False, seed=1340),                    # left = right slot
    "c1": dict(_TINY, C=1, seed=1351),                                # L = 3 (seed 1350: fp32 reference 6.4e-5 from fp64)
    "b1": dict(_TINY, B=1, bias=False, seed=1360),                    # L = 4: one impression
    "b1c1": dict(_TINY, B=1, C=1, bias=False, seed=1365),             # L = 1: a one-key softmax (a seed with a live relu)
    "long": dict(B=22, H=3, C=7, S=4, D=16, Et=12, Ec=4, heads=2, bias=True, subcat=False, p=0.0, min_len=1, seed=1370),
    # ^ L = 154: past the short kernel's 128, five key tiles, the last one ragged, two query groups
    "dropmask": dict(_TINY, p=0.25, seed=1380),
    "shipped": dict(B=4, H=25, C=5, S=50, D=768, Et=256, Ec=16, heads=16, bias=False, subcat=False, p=0.0, min_len=5, seed=1390),
}

# the state_dict contract: the flat keys of config/mind_small_LSTUR.yml plus these; initial values under torch.manual_seed
INIT = dict(config="mind_small_LSTUR", seed=0, extra=dict(model="CAUM", scoring="CAUMScoring", n_heads=16))

# tensors of more than SAMPLE_MIN elements are stored as a fixed SAMPLE_N-element sample (multiplicative hash walk)
SAMPLE_MIN, SAMPLE_N = 1024, 512


def sample(t):
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    if a.size <= SAMPLE_MIN:
        return a
    idx = (np.arange(SAMPLE_N, dtype=np.int64) * 2654435761 + 12345) % a.size
    return a.reshape(-1)[idx]


def emb_dim(c):
    return c["Et"] + c["Ec"] * (2 if c["subcat"] else 1)


def model_cfg(c):
    """The flat keys CAUM and make_model read (caum.py:33-54,117-146, make_model.py:17-32)."""
    catg = ["category_index"] + (["subcategory_index"] if c["subcat"] else [])
    return dict(model="CAUM", scoring="CAUMScoring", n_heads=c["heads"], d_backbone=c["D"], title_emb_dim=c["Et"],
                cat_emb_dim=c["Ec"], total_emb_dim=emb_dim(c), n_categories=19, n_subcategories=264, p_dropout=c["p"],
                bias=c["bias"], hist_len=c["H"], seq_len=c["S"], text_features=["title_emb"], catg_features=catg,
                user_features=[], add_features=[])


def batch(c):
    """The reference's batch dict (dataset.py:67-158) with category (and sub-category) indices."""
    from xnrs_amd import synth
    return synth.make_batch(c["seed"], c["B"], c["H"], c["C"], c["S"], c["D"], min_len=c["min_len"], n_categories=19,
                            n_subcategories=264 if c["subcat"] else 0)


def weight_seed(c):
    return c["seed"] + 1


class FixedMaskDropout(nn.Module):
    """nn.Dropout with its draw replaced by a mask that is a pure function of (seed, number of elements): in train mode
    x * keep / (1 - p), keep = (PCG64(seed).random(numel) >= p) laid out like x; identity in eval mode."""

    def __init__(self, p: float, seed: int):
        super().__init__()
        self.p, self.seed = float(p), int(seed)

    def forward(self, x):
        if not self.training:
            return x
        keep = np.random.Generator(np.random.PCG64(self.seed)).random(x.numel()) >= self.p
        mask = torch.from_numpy(keep.astype(np.float64) / (1.0 - self.p)).reshape(x.shape)
        return x * mask.to(device=x.device, dtype=x.dtype)


def fix_dropouts(model, c):
    """Put the model into the grad step's mode: everything eval; with c['p'] > 0 the tower's three dropouts become
    FixedMaskDropout modules in train mode."""
    model.eval()
    if c["p"] > 0:
        for i, name in enumerate(("dropout1", "dropout2", "dropout3")):
            setattr(model.user_encoder, name, FixedMaskDropout(c["p"], c["seed"] + 10 + i).train())
    return model
