"""Minimal DDIMScheduler with the behaviour the hot path consumes [3P diffusers==0.8.0]:
`timesteps[i]`, `add_noise(latent, noise, t)`  (optimize_token.py:25-34, ptp_utils.py:221-223), and for image sampling
`set_timesteps(n)` + `step(model_output, t, sample)` (ptp_utils.py:337-349): eta = 0; epsilon, v or sample prediction; optional
classifier-free guidance mixed into the step.  eta > 0, DPM-Solver++(2M) and its SDE form are plans of their own over this
scheduler's schedule and timestep table (ldm/samplers.py; `text2image_ldm_stable(..., sampler=)`); this class and its `step` are
what they always were.  Not built: thresholding."""
from __future__ import annotations

import torch

from .samplers import StepCoef, step_formula


PREDICTION_TYPES = ("epsilon", "v_prediction", "sample")


class DDIMScheduler:
    def __init__(self, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", num_train_timesteps=1000,
                 clip_sample=True, set_alpha_to_one=True, prediction_type="epsilon"):
        if prediction_type not in PREDICTION_TYPES:
            raise ValueError(f"prediction_type must be one of {PREDICTION_TYPES}, got {prediction_type!r}")
        self.prediction_type = prediction_type
        if beta_schedule == "scaled_linear":
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        elif beta_schedule == "linear":
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        else:
            raise NotImplementedError(beta_schedule)
        self.betas = betas
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.num_train_timesteps = num_train_timesteps
        self.clip_sample, self.set_alpha_to_one = bool(clip_sample), bool(set_alpha_to_one)
        self.final_alpha_cumprod = 1.0 if set_alpha_to_one else float(self.alphas_cumprod[0].double())
        self.num_inference_steps = num_train_timesteps
        self.timesteps = torch.arange(0, num_train_timesteps).flip(0)
        self._cache = {}

    def set_timesteps(self, num_inference_steps: int):
        self.num_inference_steps = int(num_inference_steps)
        step = self.num_train_timesteps // num_inference_steps
        self.timesteps = (torch.arange(0, num_inference_steps) * step).flip(0)

    def add_noise(self, original_samples, noise, timesteps):
        t = int(timesteps) if not torch.is_tensor(timesteps) or timesteps.dim() == 0 else int(timesteps.reshape(-1)[0])
        acp = self.alphas_cumprod[t]
        a, b = float(acp.sqrt()), float((1 - acp).sqrt())
        return a * original_samples + b * noise

    def _coefficients(self, timestep):
        """(sqrt(a_t), sqrt(1 - a_t), sqrt(a_prev), sqrt(1 - a_prev)) as host fp64 numbers; a_prev = alphas_cumprod[t - T // N] or
        final_alpha_cumprod.  `timestep` is an int or a CPU tensor, as `self.timesteps` yields: nothing is read back from a device."""
        t = int(timestep) if not torch.is_tensor(timestep) or timestep.dim() == 0 else int(timestep.reshape(-1)[0])
        prev_t = t - self.num_train_timesteps // self.num_inference_steps
        a_t = float(self.alphas_cumprod[t].double())
        a_prev = float(self.alphas_cumprod[prev_t].double()) if prev_t >= 0 else float(self.final_alpha_cumprod)
        return a_t ** 0.5, (1.0 - a_t) ** 0.5, a_prev ** 0.5, (1.0 - a_prev) ** 0.5

    def step(self, model_output, timestep, sample, *, uncond_output=None, guidance_scale=1.0, copies=1):
        """One deterministic DDIM update (eta = 0) -> {"prev_sample": x_prev}:
            m  = uncond_output + guidance_scale (model_output - uncond_output)     when `uncond_output` is given, else model_output
            (x0, eps) = ((x - sqrt(1 - a_t) m) / sqrt(a_t), m)                      prediction_type "epsilon"
                        (sqrt(a_t) x - sqrt(1 - a_t) m, sqrt(a_t) m + sqrt(1 - a_t) x)   "v_prediction"
                        (m, (x - sqrt(a_t) m) / sqrt(1 - a_t))                      "sample"
            x0 clipped to [-1, 1] when `clip_sample` (eps stays as derived before the clamp)
            x_prev = sqrt(a_prev) x0 + sqrt(1 - a_prev) eps,    a_prev = alphas_cumprod[t - T // N]  or  final_alpha_cumprod
        The coefficients are host numbers (fp64, from the CPU-side schedule); `timestep` is an int or a CPU tensor, as
        `self.timesteps` yields, so nothing is read back from the device.  A call without the new keywords on an epsilon scheduler is what it always was: the
        single pass c1 x + c2 eps (`ops.axpby`) for fp32 device tensors without clipping, the torch expression with clipping.
        With guidance, another prediction type or `copies=2`, fp32 device tensors take one kernel, `ops.ddim_step`.  Host tensors and other dtypes evaluate the formula above in torch, in the input dtype.
        `copies=2` (keyword-only, like the other two extensions): "prev_sample" is the result twice along dim 0,
        torch.cat([x_prev, x_prev]) -- the duplicated UNet input of the next guided step, written by the same kernel."""
        if copies not in (1, 2):
            raise ValueError(f"copies must be 1 or 2, got {copies!r}")
        sa, sb, pa, pb = self._coefficients(timestep)
        guided = uncond_output is not None
        on_kernel = (sample.is_cuda and sample.dtype == torch.float32 and model_output.dtype == torch.float32
                     and (not guided or uncond_output.dtype == torch.float32))
        if self.prediction_type == "epsilon" and not guided and copies == 1:       # the step as it always was
            if self.clip_sample:
                x0 = ((sample - sb * model_output) / sa).clamp(-1, 1)
                return {"prev_sample": pa * x0 + pb * model_output}
            c1, c2 = pa / sa, pb - pa * sb / sa
            if on_kernel:
                from .. import ops
                return {"prev_sample": ops.axpby(sample, model_output, c1, c2)}
            return {"prev_sample": c1 * sample + c2 * model_output}
        if on_kernel:
            from .. import ops
            return {"prev_sample": ops.ddim_step(sample, model_output, uncond_output, sa=sa, sb=sb, pa=pa, pb=pb,
                                                 guidance=float(guidance_scale), prediction=self.prediction_type,
                                                 clip=self.clip_sample, copies=copies)}
        prev, _ = step_formula(sample, model_output, uncond_output, StepCoef(sa, sb, None, pa, pb, 0, 0), guidance_scale,
                               self.prediction_type, self.clip_sample)
        return {"prev_sample": torch.cat([prev, prev]) if copies == 2 else prev}
