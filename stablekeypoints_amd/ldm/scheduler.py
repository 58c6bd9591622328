"""Minimal DDIMScheduler with the behaviour the hot path consumes [3P diffusers==0.8.0]:
`timesteps[i]`, `add_noise(latent, noise, t)`  (optimize_token.py:25-34, ptp_utils.py:221-223), and for image sampling
`set_timesteps(n)` + `step(model_output, t, sample)` (ptp_utils.py:337-349): eta = 0, epsilon prediction."""
from __future__ import annotations

import torch


class DDIMScheduler:
    def __init__(self, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", num_train_timesteps=1000,
                 clip_sample=True, set_alpha_to_one=True):
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

    def step(self, model_output, timestep, sample):
        """One deterministic DDIM update (eta = 0, epsilon prediction) -> {"prev_sample": x_prev}:
            x0 = (x - sqrt(1 - a_t) eps) / sqrt(a_t)   (clipped to [-1, 1] when `clip_sample`)
            x_prev = sqrt(a_prev) x0 + sqrt(1 - a_prev) eps,    a_prev = alphas_cumprod[t - T // N]  or  final_alpha_cumprod
        The coefficients are host numbers (fp64, from the CPU-side schedule); `timestep` is an int or a CPU tensor, as
        `self.timesteps` yields, so nothing is read back from the device.  Without clipping the update is the single pass
        c1 x + c2 eps (on the GPU: one kernel)."""
        t = int(timestep) if not torch.is_tensor(timestep) or timestep.dim() == 0 else int(timestep.reshape(-1)[0])
        prev_t = t - self.num_train_timesteps // self.num_inference_steps
        a_t = float(self.alphas_cumprod[t].double())
        a_prev = float(self.alphas_cumprod[prev_t].double()) if prev_t >= 0 else float(self.final_alpha_cumprod)
        sa, sb = a_t ** 0.5, (1.0 - a_t) ** 0.5
        pa, pb = a_prev ** 0.5, (1.0 - a_prev) ** 0.5
        if self.clip_sample:
            x0 = ((sample - sb * model_output) / sa).clamp(-1, 1)
            return {"prev_sample": pa * x0 + pb * model_output}
        c1, c2 = pa / sa, pb - pa * sb / sa
        if sample.is_cuda and sample.dtype == torch.float32 and model_output.dtype == torch.float32:
            from .. import ops
            return {"prev_sample": ops.axpby(sample, model_output, c1, c2)}
        return {"prev_sample": c1 * sample + c2 * model_output}
