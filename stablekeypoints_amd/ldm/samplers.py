"""Sampler plans of the image-sampling loop (`ptp_utils.text2image_ldm_stable(..., sampler=)`): stochastic DDIM (eta in [0, 1]),
DPM-Solver++(2M) and SDE-DPM-Solver++(2M), each as ONE linear update per step in the variance-preserving state the UNet sees.
With a = alphas_cumprod, alpha = sqrt(a), sigma = sqrt(1 - a), primes at the step's target, lambda = log(alpha / sigma),
h = lambda' - lambda and r = h_prev / h:

    m        = m_u + g (m_c - m_u)   or   m_c
    (x0,eps) from (x, m) by the prediction type with (sa, sb) = (alpha_t, sigma_t)        the three cases of DDIMScheduler.step
    (x0,eps) = (x0 - (sigma / alpha) s g, eps + s g)   with keypoint guidance: g = dE/dx, s the per-image scale (ptp_utils.py)
    x0c      = clamp(x0, -1, 1) if clip_sample else x0                                    (eps stays as derived before the clamp)
    y        = cx x + c0 x0c + ce eps + c1 x0_prev + cn noise,        x0_prev = the previous step's x0c

    "ddim"         s = eta sqrt((1 - a') / (1 - a)) sqrt(1 - a / a');   c0 = alpha', ce = sqrt(1 - a' - s^2), cn = s, cx = c1 = 0
    "dpm++2m"      cx = sigma' / sigma, cD = -alpha' expm1(-h);  y = cx x + cD D
    "dpm++2m-sde"  cx = (sigma' / sigma) exp(-h), cD = alpha' (1 - exp(-2h)), cn = sigma' sqrt(1 - exp(-2h));  y = cx x + cD D + cn noise
      D = x0c on the first step, on the last step (lower_order_final) and whenever sigma' == 0 -- there h is infinite and the
          limit is written out: cx = cn = 0, cD = alpha';
      D = (1 + 1 / (2r)) x0c - (1 / (2r)) x0_prev on every other step, so c0 = cD (1 + 1 / (2r)), c1 = -cD / (2r).

A plan is host arithmetic in fp64 on the CPU-side schedule, as `DDIMScheduler._coefficients` is: nothing is read back from a device.
It reads the model's scheduler and never writes to it -- `model.scheduler` stays what the optimisation path reads.  All samplers
walk the "leading" timestep table of `DDIMScheduler.set_timesteps`.  Not built: Karras sigma spacing / fractional timesteps,
Heun, UniPC, thresholding."""
from __future__ import annotations

import math
from typing import List, NamedTuple, Tuple

import torch

SAMPLERS = ("ddim", "dpm++2m", "dpm++2m-sde")


class StepCoef(NamedTuple):
    """One step's host numbers, in the order `ops.sampler_step(coef=)` and skp_sampler_step_f32 take them."""
    sa: float
    sb: float
    cx: float                                # None: no `cx x` term at all (`step_formula`; host only)
    c0: float
    ce: float
    c1: float
    cn: float


def step_formula(x, m_c, m_u, coef, guidance, prediction_type, clip, x0_prev=None, noise=None, grad=None, grad_scale=None):
    """The update at the top of this file in torch, in the dtype of its inputs -> (y, x0c): what the step kernel
    (`ops.sampler_step`, `ops.ddim_step`) computes, for host tensors and other dtypes.  `m_u` None: no guidance.  A term whose tensor
    is absent is not evaluated, and neither is `cx x` when `coef.cx` is None (the DDIM form y = c0 x0c + ce eps of
    `DDIMScheduler.step`; a `0 * x` there would turn a -0 into +0 and an infinite x into NaN).  `grad` (shaped like x) with
    `grad_scale` ([rows], one per leading row of x): the gradient term of keypoint guidance, applied to (x0, eps) before the clamp."""
    m = m_c if m_u is None else m_u + guidance * (m_c - m_u)
    if prediction_type == "epsilon":
        x0, eps = (x - coef.sb * m) / coef.sa, m
    elif prediction_type == "v_prediction":
        x0, eps = coef.sa * x - coef.sb * m, coef.sa * m + coef.sb * x
    else:
        x0, eps = m, (x - coef.sa * m) / coef.sb
    if grad is not None:
        sg = grad_scale.reshape((-1,) + (1,) * (grad.dim() - 1)) * grad
        x0, eps = x0 - (coef.sb / coef.sa) * sg, eps + sg
    if clip:
        x0 = x0.clamp(-1, 1)
    y = coef.c0 * x0 + coef.ce * eps if coef.cx is None else coef.cx * x + coef.c0 * x0 + coef.ce * eps
    if x0_prev is not None:
        y = y + coef.c1 * x0_prev
    if noise is not None:
        y = y + coef.cn * noise
    return y, x0


STEP_ROW = 8                                 # SKP_STEP_ROW of include/skp_sampler_graph.h


def pack_step_table(coefs, guidance: float = 1.0) -> torch.Tensor:
    """The rows of a plan as the device-row step kernels read them (include/skp_sampler_graph.h): float32 [steps, STEP_ROW] on the
    host, row i = (sa, sb, cx, c0, ce, c1, cn, guidance) of `coefs[i]` -- fp64 host numbers, each rounded to float32 ONCE, which is
    what the by-value entries make of the same numbers in their argument lists.  A `cx` of None (the DDIM form) is stored as 0."""
    rows = [[float(0.0 if v is None else v) for v in c] + [float(guidance)] for c in coefs]
    return torch.tensor(rows, dtype=torch.float64).reshape(len(rows), STEP_ROW).to(torch.float32)


def is_stochastic(kind: str, eta: float = 0.0) -> bool:
    return kind == "dpm++2m-sde" or (kind == "ddim" and eta > 0)


class SamplerPlan:
    """`SamplerPlan(scheduler, kind, eta).plan(n)` -> (timesteps, [StepCoef] * n).  `order=1` forces the first-order update on
    every step of the two multistep solvers (what they do on their first and last step anyway)."""

    def __init__(self, scheduler, kind: str = "ddim", eta: float = 0.0, order: int = 2):
        if kind not in SAMPLERS:
            raise ValueError(f"sampler must be one of {SAMPLERS}, got {kind!r}")
        eta = float(eta)
        if not 0.0 <= eta <= 1.0:                                # (NaN fails too)
            raise ValueError(f"eta must be in [0, 1], got {eta!r}")
        if eta != 0 and kind != "ddim":
            raise ValueError(f"eta = {eta!r} belongs to sampler \"ddim\"; {kind!r} has no such parameter")
        if order not in (1, 2):
            raise ValueError(f"order must be 1 or 2, got {order!r}")
        self.kind, self.eta, self.order = kind, eta, order
        self.alphas_cumprod = scheduler.alphas_cumprod.detach().to("cpu", torch.float64)       # a copy: the scheduler is not touched
        self.final_alpha_cumprod = float(scheduler.final_alpha_cumprod)
        self.num_train_timesteps = int(scheduler.num_train_timesteps)
        self.prediction_type = scheduler.prediction_type
        self.clip_sample = bool(scheduler.clip_sample)

    @property
    def stochastic(self) -> bool:
        return is_stochastic(self.kind, self.eta)

    def plan(self, num_inference_steps: int) -> Tuple[torch.Tensor, List[StepCoef]]:
        n = int(num_inference_steps)
        if n < 1:
            raise ValueError(f"num_inference_steps must be at least 1, got {num_inference_steps!r}")
        stride = self.num_train_timesteps // n
        timesteps = (torch.arange(0, n) * stride).flip(0)        # DDIMScheduler.set_timesteps' table
        rows, h_prev = [], None
        for i, t in enumerate(timesteps.tolist()):
            a = float(self.alphas_cumprod[t])
            a_p = float(self.alphas_cumprod[t - stride]) if t - stride >= 0 else self.final_alpha_cumprod
            al, sg, al_p, sg_p = math.sqrt(a), math.sqrt(1.0 - a), math.sqrt(a_p), math.sqrt(1.0 - a_p)
            if self.kind == "ddim":
                s = self.eta * math.sqrt((1.0 - a_p) / (1.0 - a)) * math.sqrt(1.0 - a / a_p)
                rows.append(StepCoef(al, sg, 0.0, al_p, math.sqrt(max(1.0 - a_p - s * s, 0.0)), 0.0, s))
                continue
            if sg_p == 0.0:                                      # h is infinite: the limit of either solver
                rows.append(StepCoef(al, sg, 0.0, al_p, 0.0, 0.0, 0.0))
                h_prev = None
                continue
            h = math.log(al_p / sg_p) - math.log(al / sg)
            if self.kind == "dpm++2m":
                cx, cd, cn = sg_p / sg, -al_p * math.expm1(-h), 0.0
            else:
                cx, cd, cn = sg_p / sg * math.exp(-h), -al_p * math.expm1(-2.0 * h), sg_p * math.sqrt(-math.expm1(-2.0 * h))
            if self.order == 1 or i == 0 or i == n - 1 or h_prev is None:
                c0, c1 = cd, 0.0
            else:
                r = h_prev / h
                c0, c1 = cd * (1.0 + 0.5 / r), -cd * 0.5 / r
            rows.append(StepCoef(al, sg, cx, c0, 0.0, c1, cn))
            h_prev = h
        return timesteps, rows
