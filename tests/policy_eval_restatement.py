"""A numpy float64 restatement of the policy evaluation pass (csrc/gemx_policy_eval.hip): the input construction of both modes and of
`last`, and the heads in the kernel's operation order (include/gemx.h).  A helper, not a test; the MLP and its per-output error bound
are tests/policy_restatement.forward."""
import numpy as np

import policy_restatement as pr

HALF_LOG_2PI, HALF_LOG_2PIE, LOG_2 = 0.9189385332046727, 1.4189385332046727, 0.6931471805599453


def inputs(traj, columns, mode="seen", last=False, obs0=None, ended=None, reset_obs=None, references=None, last_references=None, refs=None, shown0=None,
           references_next=None):
    """x [K (+1 with last), N, n_in] float64.  seen: o[0] = obs0, o[k] = traj[k-1] or reset_obs where ended[k-1]; r[k] = references[k]
    (row K: last_references), or r[0] = shown0, r[k] = refs[k-1] in the complete form.  next: o = traj, r = refs or references_next."""
    traj = traj.astype(np.float64)
    K = traj.shape[0]
    if mode == "next":
        o, r = traj, (refs if refs is not None else references_next)
    else:
        o = np.concatenate([obs0[None].astype(np.float64), traj[: K if last else K - 1]], axis=0)
        for k in range(1, o.shape[0]):
            e = ended[k - 1].astype(bool)
            o[k][e] = (reset_obs.astype(np.float64)[e] if reset_obs.ndim == 2 else reset_obs.astype(np.float64))
        if refs is not None:
            r = np.concatenate([shown0[None], refs[: K if last else K - 1]], axis=0)
        elif references is not None:
            r = np.concatenate([references, last_references[None]], axis=0) if last else references
        else:
            r = None
    x = o[:, :, columns]
    return x if r is None else np.concatenate([x, r.astype(np.float64)], axis=2)


def categorical(out, actions):
    """-> (log_prob, entropy) [..]: m = max; s = sum exp(out_i - m) ascending from 0; lse = m + log s; l_i = out_i - lse; -(sum exp(l_i) l_i)."""
    z = out.astype(np.float64)
    n = z.shape[-1]
    m = z.max(axis=-1)
    s = np.zeros_like(m)
    for i in range(n):
        s = s + np.exp(z[..., i] - m)
    lse = m + np.log(s)
    h = np.zeros_like(m)
    lp = np.full_like(m, np.nan)
    for i in range(n):
        l = z[..., i] - lse
        h = h + np.exp(l) * l
        lp = np.where(actions == i, l, lp)
    return lp, -h


def gaussian(out, pre_squash, log_std, squash_correction=False):
    z, u, ls = out.astype(np.float64), pre_squash.astype(np.float64), log_std.astype(np.float64)
    lp, c, h = np.zeros(z.shape[:-1]), np.zeros(z.shape[:-1]), np.zeros(z.shape[:-1])
    for j in range(z.shape[-1]):
        sg = np.exp(ls[j])
        d = u[..., j] - z[..., j]
        q = (d * d) / (2.0 * (sg * sg))
        lp = lp + (((-q) - ls[j]) - HALF_LOG_2PI)
        h = h + (ls[j] + HALF_LOG_2PIE)
        if squash_correction:
            t = -2.0 * u[..., j]
            sp = np.maximum(t, 0.0) + np.log1p(np.exp(-np.abs(t)))
            c = c + 2.0 * ((LOG_2 - u[..., j]) - sp)
    return (lp - c if squash_correction else lp), h


def tanh_correction(u):
    """One component of the change of variables, log(1 - tanh(u)^2), as the Gaussian head computes it."""
    u = np.asarray(u, dtype=np.float64)
    t = -2.0 * u
    return 2.0 * ((LOG_2 - u) - (np.maximum(t, 0.0) + np.log1p(np.exp(-np.abs(t)))))


def value(out):
    return out.astype(np.float64)[..., 0]


forward = pr.forward
