"""Test infrastructure: the DPM-Solver++ contract of INTEGRATION.md ("DPM-Solver++ scheduler", rules 1-6, a restatement of diffusers'
DPMSolverSinglestepScheduler with its defaults) written out again in fp64 torch, directly from the rules.  It deliberately imports
nothing from the package's dpm_solver module, so that the tests comparing the two are not circular."""
import math

import torch

F64 = torch.float64


def sd15_alphas_cumprod(n=1000, linear_start=0.00085, linear_end=0.012):
    """The SD-1.5 "scaled_linear" schedule: betas = linspace(sqrt(start), sqrt(end), n) ** 2, alphas_cumprod = cumprod(1 - betas)."""
    betas = torch.linspace(linear_start ** 0.5, linear_end ** 0.5, n, dtype=F64) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def timesteps(S, T=1000):
    """Rule 1: linspace(0, T - 1, S + 1), rounded half to even, descending, without the trailing 0."""
    return [int(v) for v in torch.round(torch.linspace(0, T - 1, S + 1, dtype=F64)).flip(0)[:-1]]


def orders(n):
    """Rule 2, element by element: the last step is order 1, and so is the one before it when n is even; otherwise 1, 2, 1, 2, ..."""
    out = []
    for k in range(n):
        if k == n - 1 or (n % 2 == 0 and k == n - 2):
            out.append(1)
        else:
            out.append(1 if k % 2 == 0 else 2)
    return out


def img2img(S, strength):
    """Rule 6: (n, t_first, the timesteps run, their orders)."""
    if not 0 < strength <= 1:
        raise ValueError(strength)
    n = min(int(S * strength), S)
    if n == 0:
        raise ValueError(strength)
    ts = timesteps(S)[S - n:]
    return n, ts[0], ts, orders(n)


def alpha_sigma(ac, t):
    """(alpha, sigma) of timestep t; t = None is the final point (1, 0)."""
    if t is None:
        return 1.0, 0.0
    a = float(ac[t])
    return math.sqrt(a), math.sqrt(1.0 - a)


def lam(ac, t):
    a, s = alpha_sigma(ac, t)
    return math.log(a) - math.log(s)


def coefficients(ac, ts, ords):
    """Rules 4 and 5 as per-step coefficient tuples (alpha_s, sigma_s, c_base, c0, c1, uses_block_start):
    x_{i+1} = c_base x_base + c0 x0_i + c1 x0_prev, with x_base = x_i (order 1) or x_{i-1} (order 2)."""
    out = []
    for i, (t, o) in enumerate(zip(ts, ords)):
        a_i, s_i = alpha_sigma(ac, t)
        if i == len(ts) - 1:
            out.append((a_i, s_i, 0.0, 1.0, 0.0, False))
            continue
        t1 = ts[i + 1]
        a1, s1 = alpha_sigma(ac, t1)
        if o == 1:
            h = lam(ac, t1) - lam(ac, t)
            out.append((a_i, s_i, s1 / s_i, a1 * (1.0 - math.exp(-h)), 0.0, False))
        else:
            tb = ts[i - 1]
            h = lam(ac, t1) - lam(ac, tb)
            r0 = (lam(ac, t) - lam(ac, tb)) / h
            w = a1 * (1.0 - math.exp(-h))
            # x0_{i-1} + (x0_i - x0_{i-1}) / (2 r0) = (1 - 1/(2 r0)) x0_{i-1} + 1/(2 r0) x0_i
            out.append((a_i, s_i, s1 / alpha_sigma(ac, tb)[1], w / (2.0 * r0), w * (1.0 - 1.0 / (2.0 * r0)), True))
    return out


def guide_scales(n, g):
    """Rule 3: DDIMSampler.guide_scales(n, g) (linear annealing from max(2, g), constant for a scalar g); one step takes the first."""
    if isinstance(g, (list, tuple)):
        hi, lo = g
    else:
        hi = lo = max(2.0, g)
    if n == 1:
        return [hi]
    return [hi - (hi - lo) * i / (n - 1) for i in range(n)]


def run(ac, ts, ords, x_T, eps_fn, on_step=None, n_steps=None):
    """Rules 3-5 as a loop in fp64: eps_fn(x, t, i) -> the guided epsilon at step i.  Returns the list x_0 = x_T, x_1, ..., x_n and the
    list of x0 predictions.  on_step(i, x_i, e_i, x0_i) is called at each step; n_steps stops the run after that many steps."""
    xs, x0s = [x_T.to(F64)], []
    for i, (t, o) in enumerate(zip(ts, ords)):
        if n_steps is not None and i == n_steps:
            break
        a_i, s_i = alpha_sigma(ac, t)
        e = eps_fn(xs[i], t, i).to(F64)
        x0 = (xs[i] - s_i * e) / a_i
        x0s.append(x0)
        if on_step:
            on_step(i, xs[i], e, x0)
        if i == len(ts) - 1:
            xs.append(x0)
            continue
        t1 = ts[i + 1]
        a1, s1 = alpha_sigma(ac, t1)
        if o == 1:
            h = lam(ac, t1) - lam(ac, t)
            xs.append((s1 / s_i) * xs[i] + a1 * (1.0 - math.exp(-h)) * x0)
        else:
            assert i >= 1 and ords[i - 1] == 1
            tb = ts[i - 1]
            h = lam(ac, t1) - lam(ac, tb)
            r0 = (lam(ac, t) - lam(ac, tb)) / h
            s_b = alpha_sigma(ac, tb)[1]
            xs.append((s1 / s_b) * xs[i - 1] + a1 * (1.0 - math.exp(-h)) * (x0s[i - 1] + (x0 - x0s[i - 1]) / (2.0 * r0)))
    return xs, x0s


# ---- a Gaussian data model: x0 ~ N(mu, s^2) element-wise, for which epsilon and the probability-flow ODE are closed-form
def gaussian_eps(x, alpha, sigma, mu, s):
    """E[eps | x_t = x] for x_t = alpha x0 + sigma eps: sigma (x - alpha mu) / (alpha^2 s^2 + sigma^2)."""
    return sigma * (x - alpha * mu) / (alpha * alpha * s * s + sigma * sigma)


def gaussian_flow(x_T, a_T, s_T, alpha, sigma, mu, s):
    """The probability-flow ODE solution from (a_T, s_T, x_T) at (alpha, sigma)."""
    return alpha * mu + math.sqrt(alpha * alpha * s * s + sigma * sigma) / math.sqrt(a_T * a_T * s * s + s_T * s_T) * (x_T - a_T * mu)
