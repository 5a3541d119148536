"""Higher-order samplers as PROGRAMS for the engine's table-driven update (csrc/elementwise.hip, solver_step_kernel).

The engine knows one linear update per model evaluation j,

    g   = ga * x + gb * v
    x'  = cx * x + cs * xs + c0 * g + c1 * hist[h1_slot] + c2 * hist[h2_slot]

with `xs` a saved iterate and `hist` two history slots; row j of `coef` = (cx, cs, c0, c1, c2, ga, gb, 0) and of `ctl` = (save_xs, w_slot,
h1_slot, h2_slot) say what evaluation j does (save_xs: keep the pre-update x; w_slot >= 0: keep g in that slot; a slot of -1 or a coefficient
of 0 means the term is absent).  Which solver runs is decided here, on the host, in float64: the flow ODE is dx/dsigma = v(x, sigma), and
`sigmas` is the descending list of the N + 1 times of N user steps.

`times[j]` is the model time of evaluation j and `times[j + 1]` the time of the iterate it produces (len(times) = evaluations + 1);
`step_of_eval[j]` is the user step evaluation j belongs to.

A step ONTO sigma = 0 is, for every solver, the single evaluation x' = x - sigma_i * v = D (the data prediction), written cx = 0, ga = 1,
gb = -sigma_i, c0 = 1: Euler's last step in the form that leaves no trace of x's rounding in the coefficient of D (diffusers' Heun ends with
the same first-order step).  Pure Python: no device, no torch."""
import math
from typing import List, NamedTuple, Sequence, Tuple

SAMPLERS = ("euler", "heun", "midpoint", "ab2", "dpmpp_2m")
SIGMA_SCHEDULES = (None, "karras", "exponential")
KARRAS_RHO = 7.0


class SolverProgram(NamedTuple):
    times: Tuple[float, ...]                 # evaluations + 1
    coef: Tuple[Tuple[float, ...], ...]      # [evaluations][8] = cx, cs, c0, c1, c2, ga, gb, 0
    ctl: Tuple[Tuple[int, ...], ...]         # [evaluations][4] = save_xs, w_slot, h1_slot, h2_slot
    step_of_eval: Tuple[int, ...]            # [evaluations] -> user step


def _row(cx=0.0, cs=0.0, c0=0.0, c1=0.0, c2=0.0, ga=0.0, gb=0.0):
    return (float(cx), float(cs), float(c0), float(c1), float(c2), float(ga), float(gb), 0.0)


def _ctl(save_xs=0, w_slot=-1, h1_slot=-1, h2_slot=-1):
    return (int(save_xs), int(w_slot), int(h1_slot), int(h2_slot))


def check_sigmas(sigmas: Sequence[float]) -> List[float]:
    """the times of a program: finite, strictly descending, every one but the last > 0, the last >= 0 -> a list of floats"""
    try:
        s = [float(v) for v in sigmas]
    except (TypeError, ValueError):
        raise ValueError(f"fluxmi: sigmas={sigmas!r}: expected a list of numbers") from None
    if not s:
        raise ValueError("fluxmi: an empty sigma list")
    if not all(math.isfinite(v) for v in s):
        raise ValueError("fluxmi: sigmas must be finite")
    if any(b >= a for a, b in zip(s[:-1], s[1:])):
        raise ValueError("fluxmi: sigmas must be strictly descending")
    if s[-1] < 0.0 or any(v <= 0.0 for v in s[:-1]):
        raise ValueError("fluxmi: sigmas must be positive (only the last may be 0)")
    return s


def custom_sigmas(sigmas: Sequence[float]) -> List[float]:
    """a request's own `sigmas=` list (the argument of diffusers' FluxPipeline): finite, strictly descending, in (0, 1], with or without a
    trailing 0 -> the timestep list, ending at 0"""
    s = check_sigmas(sigmas)
    if s[-1] == 0.0:
        s = s[:-1]
    if not s:
        raise ValueError("fluxmi: sigmas holds no step (only the trailing 0)")
    if s[0] > 1.0:
        raise ValueError(f"fluxmi: sigmas must lie in (0, 1], got {s[0]}")
    return s + [0.0]


def sigma_schedule(kind, base: Sequence[float]) -> List[float]:
    """Re-space a schedule between its first and its last non-zero sigma, keeping the number of values (diffusers' _convert_to_karras with
    rho 7 / _convert_to_exponential); a trailing 0 stays where it is.  None keeps the schedule as it is."""
    if kind not in SIGMA_SCHEDULES:
        raise ValueError(f"fluxmi: sigma_schedule={kind!r}: expected one of {SIGMA_SCHEDULES}")
    s = check_sigmas(base)
    if kind is None:
        return s
    tail = [0.0] if s[-1] == 0.0 else []
    body = s[:-1] if tail else s
    n = len(body)
    if n < 2:
        return s
    hi, lo = body[0], body[-1]
    ramp = [i / (n - 1) for i in range(n)]
    if kind == "karras":
        a, b = hi ** (1.0 / KARRAS_RHO), lo ** (1.0 / KARRAS_RHO)
        out = [(a + r * (b - a)) ** KARRAS_RHO for r in ramp]
    else:
        a, b = math.log(hi), math.log(lo)
        out = [math.exp(a + r * (b - a)) for r in ramp]
    out[0], out[-1] = hi, lo  # the endpoints are the request's own, bit for bit
    return out + tail


def build_program(name: str, sigmas: Sequence[float]) -> SolverProgram:
    """`name` in SAMPLERS, `sigmas` the N + 1 descending times of N user steps -> the program (module docstring)."""
    if name not in SAMPLERS:
        raise ValueError(f"fluxmi: sampler={name!r}: expected one of {SAMPLERS}")
    s = check_sigmas(sigmas)
    N = len(s) - 1
    times, coef, ctl, soe = [], [], [], []

    def emit(t, row, c, i):
        times.append(t)
        coef.append(row)
        ctl.append(c)
        soe.append(i)

    for i in range(N):
        a, b = s[i], s[i + 1]
        dt = b - a
        last = i == N - 1
        if b == 0.0:  # onto sigma = 0: x' = D, for every solver
            emit(a, _row(c0=1.0, ga=1.0, gb=-a), _ctl(), i)
        elif name == "euler":
            emit(a, _row(cx=1.0, gb=1.0, c0=dt), _ctl(), i)
        elif name == "heun":
            if last:  # diffusers' FlowMatchHeunDiscreteScheduler ends first-order
                emit(a, _row(cx=1.0, gb=1.0, c0=dt), _ctl(), i)
            else:
                emit(a, _row(cx=1.0, gb=1.0, c0=dt), _ctl(save_xs=1, w_slot=0), i)            # x~ = x + dt v1; keep x, v1
                emit(b, _row(cs=1.0, gb=1.0, c0=0.5 * dt, c1=0.5 * dt), _ctl(h1_slot=0), i)   # x' = xs + dt/2 v2 + dt/2 v1
        elif name == "midpoint":
            emit(a, _row(cx=1.0, gb=1.0, c0=0.5 * dt), _ctl(save_xs=1), i)                    # x~ = x + dt/2 v1 at t + dt/2
            emit(a + 0.5 * dt, _row(cs=1.0, gb=1.0, c0=dt), _ctl(), i)                        # x' = xs + dt v2
        elif name == "ab2":
            w_slot = -1 if last else i % 2
            if i == 0:
                emit(a, _row(cx=1.0, gb=1.0, c0=dt), _ctl(w_slot=w_slot), i)
            else:
                w = dt / (2.0 * (a - s[i - 1]))
                emit(a, _row(cx=1.0, gb=1.0, c0=dt * (1.0 + w), c1=-dt * w), _ctl(w_slot=w_slot, h1_slot=(i - 1) % 2), i)
        else:  # dpmpp_2m: exponential integrator in lambda = -log sigma on D = x - sigma v
            cx = b / a
            w_slot = -1 if last else i % 2
            if i == 0:
                emit(a, _row(cx=cx, ga=1.0, gb=-a, c0=1.0 - cx), _ctl(w_slot=w_slot), i)
            else:
                r = (math.log(s[i - 1]) - math.log(a)) / (math.log(a) - math.log(b))  # (lambda_i - lambda_{i-1}) / (lambda_{i+1} - lambda_i)
                emit(a, _row(cx=cx, ga=1.0, gb=-a, c0=(1.0 - cx) * (1.0 + 0.5 / r), c1=-(1.0 - cx) * 0.5 / r),
                     _ctl(w_slot=w_slot, h1_slot=(i - 1) % 2), i)
    times.append(s[-1])
    return SolverProgram(tuple(times), tuple(coef), tuple(ctl), tuple(soe))
