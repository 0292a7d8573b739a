"""Generator parameters of the LSTUR model fixtures (lstur_model.json / lstur_model.npz, written by make_golden_lstur.py): the
reference's LSTUR (xnrs/models/full_models/lstur.py:9-159) in eval mode and inside the MSE grad step
(training.py:97-113,376-393).  Inputs and weights regenerate from these seeds through xnrs_amd.synth on every machine; the
fixtures hold outputs only.  (lstur.npz / cases.py hold the news encoder's own fixture and are not touched by this.)"""
import numpy as np
import torch

# (long_term_method, long_short_term_method) pairs the reference can run; ('mean', 'con') -- the shipped YAML's -- constructs
# and then fails at scoring (408 against 272 columns, SURVEY.md finding 5)
COMBOS = (("embedding", "ini"), ("embedding", "con"), ("embedding", "lt_only"), ("mean", "ini"), ("mean", "lt_only"))

# tiny: st_hist_len < hist_len, ragged histories (empty trailing slots), uid 0 (the padding row) and a repeated uid
# shipped: config/mind_small_LSTUR.yml's shapes (25 x 50 x 768 tokens, E = 256 + 16, st_hist_len = 25) at a small B / n_users
SHAPES = {
    "tiny": dict(B=4, H=6, st=4, C=3, S=6, D=16, Et=8, Ec=4, n_users=10, uids=[2, 0, 2, 5], seed=1200, min_len=1),
    "shipped": dict(B=3, H=25, st=25, C=5, S=50, D=768, Et=256, Ec=16, n_users=40, uids=[7, 0, 31], seed=1210, min_len=5),
}


def _case(shape, ltm, lstm, scoring="dot", hole=False):
    return dict(SHAPES[shape], ltm=ltm, lstm=lstm, scoring=scoring, hole=hole)


CASES = {f"tiny/{a}_{b}": _case("tiny", a, b) for a, b in COMBOS}
# a history mask with a HOLE: slot 1 of row 0 is an all-masked news in front of real ones -- the GRU still reads the first
# sum(mask) slots of the row, the hole included (pack_padded_sequence, lstur.py:139-145)
CASES["tiny/hole_embedding_ini"] = _case("tiny", "embedding", "ini", hole=True)
CASES["tiny/hole_mean_ini"] = _case("tiny", "mean", "ini", hole=True)
CASES["tiny/bilin"] = _case("tiny", "embedding", "con", scoring="bilin")
CASES["tiny/fc"] = _case("tiny", "embedding", "con", scoring="fc")
CASES["shipped/embedding_con"] = _case("shipped", "embedding", "con")
CASES["shipped/mean_ini"] = _case("shipped", "mean", "ini")

# the state_dict contract of mind_small_LSTUR.yml at a small n_users; initial values under torch.manual_seed(INIT["seed"])
INIT = dict(config="mind_small_LSTUR", n_users=50, seed=0)

# tensors of more than SAMPLE_MIN elements are stored as a fixed SAMPLE_N-element sample (multiplicative hash walk)
SAMPLE_MIN, SAMPLE_N = 1024, 512


def sample(t):
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    if a.size <= SAMPLE_MIN:
        return a
    idx = (np.arange(SAMPLE_N, dtype=np.int64) * 2654435761 + 12345) % a.size
    return a.reshape(-1)[idx]


def model_cfg(c):
    """The flat YAML keys LSTUR and make_model read (lstur.py:85-116,164-189, make_model.py:17-32); both dropouts 0."""
    return dict(model="LSTUR", base_model="LSTUR", scoring=c["scoring"], long_term_method=c["ltm"],
                long_short_term_method=c["lstm"], n_users=c["n_users"], d_backbone=c["D"], title_emb_dim=c["Et"],
                cat_emb_dim=c["Ec"], total_emb_dim=c["Et"] + c["Ec"], n_categories=19, n_subcategories=264,
                p_dropout=0.0, p_user_dropout=0.0, bias=False, hist_len=c["H"], st_hist_len=c["st"], seq_len=c["S"],
                text_features=["title_emb"], catg_features=["category_index"], user_features=["user_index"], add_features=[])


def batch(c):
    """The reference's batch dict (dataset.py:67-158) with category indices and user_features.other.user_index:(B,1)."""
    from xnrs_amd import synth
    b = synth.make_batch(c["seed"], c["B"], c["H"], c["C"], c["S"], c["D"], min_len=c.get("min_len", 1), n_categories=19)
    if c["hole"]:
        hx, hm = b["user_features"]["history"]["title_emb"]
        hm[:, 0] = 1.0   # every row has at least two real slots around the hole ...
        hm[:, 2] = 1.0
        hm[0, 1] = 0.0   # ... and row 0 an all-masked news between them
    b["user_features"]["other"] = {"user_index": torch.tensor(c["uids"], dtype=torch.int32).reshape(-1, 1)}
    return b


def weight_seed(c):
    return c["seed"] + 1
