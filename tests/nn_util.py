"""What the restatements of the neural rules share (policy_util, joint_policy_util and dqn_util re-export these under
their old names): the splitmix64 finalizer in Python integers and in NumPy uint64, its constants, the 24-bit uniform of a
mixed word, the float64 parameter dict of a module and the logistic function.  Only what was identical lives here: a helper
that differs in a shape or an argument (the per-row uniforms and Gumbels, ``scale_params``, ``params_of``, ``logp_of`` /
``choose``, dqn_util's masking ``mix``) stays in its module.  Nothing here imports the library."""

from __future__ import annotations

import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def mix_int(x: int) -> int:
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def _mix_np(x):
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def uniform24_int(x: int) -> float:
    """The top 24 bits of a mixed word as a uniform in (0, 1): 25 significant bits, exact in float64."""
    return ((x >> 40) + 0.5) * 2.0 ** -24


def uniform24_np(x) -> np.ndarray:
    return ((x >> np.uint64(40)).astype(np.float64) + 0.5) * 2.0 ** -24


def params64(module) -> dict:
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in module.state_dict().items()}


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))
