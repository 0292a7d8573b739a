"""Generator parameters of the scorer fixtures (scorers.json / scorers.npz, written by make_golden_scorers.py): the
bilinear and MLP scorers of the reference (xnrs/models/components/scoring.py:41-102), alone and inside the train step.
Inputs and weights regenerate from these seeds through xnrs_amd.synth on every machine; the fixtures hold outputs only."""
import numpy as np
import torch

# the scorer alone: u:(B,1,E), c:(B,N,E), upstream gradient g:(B,N,1); weights synth.fill_state_dict(shapes, seed + 1)
SCORER = {
    "bilin_bias": dict(kind="bilin", B=3, N=4, E=8, bias=True, normalize=False, seed=700),
    "bilin_nobias": dict(kind="bilin", B=2, N=5, E=12, bias=False, normalize=False, seed=701),
    "bilin_norm_bias": dict(kind="bilin", B=3, N=4, E=8, bias=True, normalize=True, seed=702),
    "bilin_norm_nobias": dict(kind="bilin", B=4, N=3, E=20, bias=False, normalize=True, seed=703),
    "fc_bias": dict(kind="fc", B=3, N=4, E=8, H=4, bias=True, seed=710),
    "fc_nobias": dict(kind="fc", B=2, N=5, E=12, H=6, bias=False, seed=711),
    "fc_odd_h": dict(kind="fc", B=3, N=2, E=10, H=5, bias=True, seed=712),
}

# the whole-model grad step in the reference's call order (training.py:402-431): relu scores -> MSE against the targets,
# + lambda * InfoNCE over get_user_embeddings; weights synth.fill_state_dict(shapes, seed + 1)
STEP = {
    "standard_cl": dict(model="standard", B=16, H=4, C=2, S=50, D=768, h=16, E=256, bias=False, seed=720, min_len=5,
                        temperature=0.08, lambda_cl=0.1),
    "nrms_tiny": dict(model="NRMS", B=4, H=3, C=3, S=8, D=32, h=4, E=16, bias=False, seed=730, temperature=0.08, lambda_cl=0.1),
    "naml_tiny": dict(model="NAML", B=3, H=3, C=3, S=8, D=32, h=4, E=16, bias=False, seed=740, temperature=0.08, lambda_cl=0.1),
}
STEP_SCORERS = ("bilin", "fc")

# the scorer's initial parameters under torch.manual_seed(INIT_SEED), at a small E
INIT = dict(E=6, seed=0)

# gradients of more than SAMPLE_MIN elements are stored as a fixed SAMPLE_N-element sample (multiplicative hash walk)
SAMPLE_MIN, SAMPLE_N = 1024, 512


def sample_idx(numel: int):
    if numel <= SAMPLE_MIN:
        return None
    return (np.arange(SAMPLE_N, dtype=np.int64) * 2654435761 + 12345) % numel


def sample(t):
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    idx = sample_idx(a.size)
    return a if idx is None else a.reshape(-1)[idx]


def scorer_inputs(c):
    """-> (u:(B,1,E), c:(B,N,E), g:(B,N,1)) fp32 CPU tensors."""
    from xnrs_amd import synth
    rng = synth.rng_for(c["seed"])
    B, N, E = c["B"], c["N"], c["E"]
    u = torch.from_numpy(rng.standard_normal((B, 1, E)).astype(np.float32))
    cv = torch.from_numpy(rng.standard_normal((B, N, E)).astype(np.float32))
    g = torch.from_numpy(rng.standard_normal((B, N, 1)).astype(np.float32))
    return u, cv, g


def step_cfg(c, scoring):
    from xnrs_amd import synth
    return dict(synth.model_cfg(c), scoring=scoring)


def step_labels(B):
    """Impression themes of a step: three themes in a fixed pattern (InfoNCE needs positives)."""
    return torch.tensor([(3 * i) % 5 % 3 for i in range(B)])
