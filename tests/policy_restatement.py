"""The MLP actor of the policy rollout (csrc/gemx_policy.hip) restated in float64 with numpy, with the forward-error bound of the
kernel's fp32 arithmetic computed alongside.  The input of step k is the rollout's OWN rows (traj[k-1], or the reset observation where
ended[k-1]; obs0 at k = 0; references[k]; noise[k]), so every step is judged on what the kernel itself saw.

The bound: an fp32 dot product of fan-in n started from the bias, evaluated as an fma chain, has |fl - exact| <= gamma_{n+1} sum |w_i x_i|
(+ |b|), gamma_m = m u / (1 - m u), u = 2^-24; an input error e propagates as |W| e; tanh (activation or squash) is 1-Lipschitz and
adds EPS_TANH, twice the device tanh's measured absolute error (profiles/policy_rollout.md); relu and clip add nothing."""
import numpy as np

U = 2.0 ** -24
EPS_TANH_MEASURED = 6.7e-8  # max |tanhf - tanh| over 2^16 points of [-10, 10] on the device (profiles/policy_rollout.md)
EPS_TANH = 2.0 * EPS_TANH_MEASURED


def gamma(m):
    return m * U / (1.0 - m * U)


def make_layers(rng, n_in, widths, scale=1.0):
    """Fixed float32 test weights: uniform in +-scale / sqrt(fan-in), biases in +-0.1."""
    layers, fan = [], n_in
    for w in widths:
        layers.append(((rng.uniform(-1, 1, (w, fan)) * scale / np.sqrt(fan)).astype(np.float32), rng.uniform(-0.1, 0.1, w).astype(np.float32)))
        fan = w
    return layers


def inputs(traj, ended, obs0, reset_obs, columns, references):
    """x [K, N, n_in] float64 from the rollout's own rows."""
    K = traj.shape[0]
    prev = np.concatenate([obs0[None], traj[:-1]], axis=0).astype(np.float64)
    if K > 1:
        prev[1:][ended[:-1].astype(bool)] = reset_obs
    x = prev[:, :, columns]
    if references is not None:
        x = np.concatenate([x, references.astype(np.float64)], axis=2)
    return x


def forward(layers, activation, x, noise=None):
    """-> (out + noise in float64, its error bound), both [..., n_out]."""
    h, err = x.astype(np.float64), np.zeros_like(x, dtype=np.float64)
    for l, (W, b) in enumerate(layers):
        W64, b64 = W.astype(np.float64), b.astype(np.float64)
        A = np.abs(W64)
        z = h @ W64.T + b64
        zerr = err @ A.T + gamma(W.shape[1] + 1) * (np.abs(h) @ A.T + np.abs(b64))
        if l + 1 < len(layers):
            if activation == "tanh":
                h, err = np.tanh(z), zerr + EPS_TANH
            else:
                h, err = np.maximum(z, 0.0), zerr
        else:
            h, err = z, zerr
    if noise is not None:
        n64 = noise.astype(np.float64)
        h, err = h + n64, err + U * np.abs(h + n64)  # one rounded addition
    return h, err


def continuous_action(out, err, squash):
    if squash == "tanh":
        return np.tanh(out), err + EPS_TANH
    return np.clip(out, -1.0, 1.0), err


def finite_action(out, err):
    """-> (float64 argmax, lowest index among maxima; excused [..] bool: the two largest logits closer than twice the bound)."""
    idx = np.argmax(out, axis=-1)
    top2 = np.sort(out, axis=-1)[..., -2:]
    return idx, (top2[..., 1] - top2[..., 0]) < 2.0 * err.max(axis=-1)


# ---- the cases of the GPU test and of the CPU margin test: one table, one construction of weights, references and noise
N_ENVS, K_STEPS = 197, 48
ENVS = {  # env id -> (state width, last layer's width, discrete, the five selected columns, bias of the last layer)
    "Cont-CC-PermExDc-v0": (5, 1, False, [2, 0, 4, 1, 3], 0.275),  # (the duty cycle that balances the back-EMF of its constant speed)
    "Finite-CC-PMSM-v0": (14, 8, True, [0, 2, 5, 6, 12], 0.0),
    "Cont-SC-SCIM-v0": (14, 3, False, [12, 0, 1, 5, 6], 0.0),
}
PLANS = {"64x64": ((64, 64), None), "16": ((16,), None), "5col": ((24, 40), "five")}  # hidden widths, column selection


def cases():
    """(env_id, M, plan, activation, squash, use_refs, use_noise): every env x M x plan x activation; noise, references and the squash
    rotate so that each env meets each plan and each activation with and without noise, with and without references, and clip and tanh
    squashes meet both activations."""
    out = []
    for env_id in ENVS:
        for im, M in enumerate((5, 1000)):
            for ip, plan in enumerate(PLANS):
                for ia, act in enumerate(("relu", "tanh")):
                    out.append((env_id, M, plan, act, "clip" if (im + ia) % 2 == 0 else "tanh", (ip + ia + im) % 2 == 1, (im + ip) % 2 == 0))
    return out


def case_data(env_id, plan, use_refs, use_noise, seed=3, n=N_ENVS, k=K_STEPS):
    """-> (layers, columns | None, references | None, noise | None) as numpy arrays, the same for the GPU and the CPU test."""
    n_state, n_logit, discrete, five, bias = ENVS[env_id]
    hidden, sel = PLANS[plan]
    columns = five if sel == "five" else None
    n_ref = 2 if use_refs else 0
    layers = make_layers(np.random.default_rng(11), (len(columns) if columns else n_state) + n_ref, tuple(hidden) + (n_logit,), scale=0.5)
    # (scale 0.5: the worst-case bound grows with the |W| row sums layer by layer while the logits' gaps keep the biases' spread; at this
    # scale the finite cases' excused share is 3e-4 at most on synthetic rows, six times below the CPU test's 0.2 % -- test_policy_cpu.py)
    layers[-1] = (layers[-1][0], (layers[-1][1] + np.float32(bias)).astype(np.float32))
    rng = np.random.default_rng(seed)
    refs = rng.uniform(-1, 1, (k, n, n_ref)).astype(np.float32) if use_refs else None
    if discrete:
        nz = rng.gumbel(size=(k, n, n_logit))
    else:  # per-lane amplitude: gentle lanes never terminate, rough ones every few steps
        nz = rng.uniform(0.0, 1.0, (1, n, 1)) ** 2 * rng.uniform(-1.0, 1.0, (k, n, n_logit))
    return layers, columns, refs, (nz.astype(np.float32) if use_noise else None)
