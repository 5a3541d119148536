"""FlowEdit (Kulikov, Kleiner, Huberman-Spiegelglas, Michaeli 2024, Algorithm 1): the host side of inversion-free text-guided editing.

The edit state z starts as the init image's latent x0 and walks an ODE whose velocity is the DIFFERENCE of the model's prediction under the
target prompt and under the source prompt, both evaluated at the same freshly noised point.  With the request's times t_0 > ... > t_T:

  steps i with T - i > n_max            are skipped (split_steps cuts the schedule; nothing runs)
  steps i with n_min < T - i <= n_max   are coupled: n_avg evaluations at t_i, each on a fresh draw, then z moves by t_{i+1} - t_i
  steps i with T - i <= n_min           are a plain Euler tail on the target branch alone

A coupled step is n_avg rows of the table the update kernel reads (csrc/flowedit.hip; include/fluxmi.h, fluxmi_flowedit_step): coef row
{w, dt, tn, 1 - tn} and ctl row {first, apply}.  Evaluation k of a step has w = 1 / n_avg (rounded to fp32, as the kernel holds it), dt =
t_{i+1} - t_i, first = (k == 0), apply = (k == n_avg - 1), and tn -- the time of the coupling that follows the update -- is t_i while the step
is still averaging and t_{i+1} once it has applied.  1 - tn is subtracted here, in double.  Nothing in this module touches the GPU.
"""
from __future__ import annotations

import struct
from typing import List, NamedTuple, Sequence, Tuple

MAX_IMAGES = 16  # one engine pass holds 32 samples: the source and the target branch of 16 images


class EditProgram(NamedTuple):
    coef: List[Tuple[float, float, float, float]]  # per evaluation: w, dt, tn, 1 - tn
    ctl: List[Tuple[int, int]]                     # per evaluation: first, apply
    times: List[float]                             # per evaluation: the model time
    step_of_eval: List[int]                        # per evaluation: the step of `timesteps` it belongs to


def _f32(v: float) -> float:
    return struct.unpack("f", struct.pack("f", v))[0]


def build_program(timesteps: Sequence[float], n_avg: int = 1) -> EditProgram:
    """the rows of the coupled steps timesteps[0] -> timesteps[1] -> ... (len(timesteps) - 1 steps, n_avg evaluations each)"""
    if isinstance(n_avg, bool) or not isinstance(n_avg, int) or n_avg < 1:
        raise ValueError(f"fluxmi: edit_n_avg={n_avg!r}: expected an integer >= 1")
    ts = [float(t) for t in timesteps]
    coef, ctl, times, step_of_eval = [], [], [], []
    w = _f32(1.0 / n_avg)
    for i in range(len(ts) - 1):
        for k in range(n_avg):
            apply = k == n_avg - 1
            tn = ts[i + 1] if apply else ts[i]
            coef.append((w, ts[i + 1] - ts[i], tn, 1.0 - tn))
            ctl.append((int(k == 0), int(apply)))
            times.append(ts[i])
            step_of_eval.append(i)
    return EditProgram(coef, ctl, times, step_of_eval)


def needs_acc(program: EditProgram) -> bool:
    """does some row store or read the fp32 accumulator (a row with first and apply keeps it in registers)?"""
    return any(not (f and a) for f, a in program.ctl)


def split_steps(num_steps: int, n_max=None, n_min: int = 0) -> Tuple[int, int]:
    """-> (a, b): of the steps 0 .. num_steps - 1, steps [0, a) are skipped, [a, b) coupled, [b, num_steps) the Euler tail.
    Step i is coupled iff n_min < num_steps - i <= n_max; n_max = None means every step."""
    T = int(num_steps)
    n_max = T if n_max is None else n_max
    for name, v in (("edit_n_max", n_max), ("edit_n_min", n_min)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"fluxmi: {name}={v!r}: expected an integer")
    if not 0 <= n_min <= n_max <= T:
        raise ValueError(f"fluxmi: edit_n_min={n_min}, edit_n_max={n_max}: expected 0 <= edit_n_min <= edit_n_max <= num_steps = {T}")
    return T - n_max, T - n_min


def edit_ids(seed: int, num_images: int, first_image: int = 0) -> List[Tuple[int, int, int, int]]:
    """the Philox ids of a request's images: (seed & 0xffffffff, seed >> 32, k, 1).  Column 3 is 1 where a stochastic sampler's is 0, so
    the two never share a draw under one seed."""
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"fluxmi: seed {seed}: expected an integer in [0, 2^64)")
    return [(seed & 0xffffffff, (seed >> 32) & 0xffffffff, first_image + k, 1) for k in range(int(num_images))]
