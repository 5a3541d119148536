"""Higher-order samplers as PROGRAMS for the engine's table-driven update (csrc/update_step.hip, solver_step_kernel).

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
the same first-order step).

Stochastic samplers (STOCHASTIC_SAMPLERS) use the eighth column, cn: the kernel's noise form (fluxmi_solver_step_noise) adds one last term
cn * z with z a standard normal drawn IN the kernel from a counter-based generator (Philox4x32-10 + Box-Muller) keyed by the request's
per-image ids and the evaluation index.  With alpha = 1 - sigma, a = sigma_i, b = sigma_{i+1} and D = x - a v (ga = 1, gb = -a):

  euler_ancestral (k-diffusion's rectified-flow form):  sd = b (1 + (b/a - 1) eta), r = sd/a, k = (1 - b)/(1 - sd),
      cx = k r,  c0 = k (1 - r),  cn = s_noise sqrt(max(0, b^2 - sd^2 (1 - b)^2 / (1 - sd)^2))
  dpmpp_2m_sde (SDE-DPM-Solver++(2M)):  E = e^{-h} = (b/a) ((1 - a)/(1 - b)), from a and b directly (a = 1 gives E = 0),
      cx = (b/a) E^eta,  cD = (1 - b)(1 - E^{1 + eta}),  cn = s_noise b sqrt(1 - E^{2 eta});
      first step or a previous sigma of 1: c0 = cD; else with r = h_{i-1}/h_i (h the log-SNR step): c1 = -cD/(2r), c0 = cD - c1,
      D kept in the alternating history slot like dpmpp_2m.

Either way a clean x0 and a noise eps are carried as x' = (1 - b) x0 + B eps + cn z with B^2 + cn^2 = b^2; eta = 0 makes every cn 0
(euler_ancestral is then Euler).  A step onto sigma = 0 stays the deterministic x' = D row.  Pure Python: no device, no torch."""
import math
import struct
from typing import List, NamedTuple, Sequence, Tuple

SAMPLERS = ("euler", "heun", "midpoint", "ab2", "dpmpp_2m")
STOCHASTIC_SAMPLERS = ("euler_ancestral", "dpmpp_2m_sde")
SIGMA_SCHEDULES = (None, "karras", "exponential")
KARRAS_RHO = 7.0


class SolverProgram(NamedTuple):
    times: Tuple[float, ...]                 # evaluations + 1
    coef: Tuple[Tuple[float, ...], ...]      # [evaluations][8] = cx, cs, c0, c1, c2, ga, gb, cn (0 for every deterministic solver)
    ctl: Tuple[Tuple[int, ...], ...]         # [evaluations][4] = save_xs, w_slot, h1_slot, h2_slot
    step_of_eval: Tuple[int, ...]            # [evaluations] -> user step


def _row(cx=0.0, cs=0.0, c0=0.0, c1=0.0, c2=0.0, ga=0.0, gb=0.0, cn=0.0):
    return (float(cx), float(cs), float(c0), float(c1), float(c2), float(ga), float(gb), float(cn))


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


def has_noise(prog: SolverProgram) -> bool:
    """does any row of the program draw noise (a non-zero cn as the fp32 table holds it)?"""
    return any(struct.unpack("f", struct.pack("f", row[7]))[0] != 0.0 for row in prog.coef)


def build_program(name: str, sigmas: Sequence[float], eta: float = 1.0, s_noise: float = 1.0) -> SolverProgram:
    """`name` in SAMPLERS or STOCHASTIC_SAMPLERS, `sigmas` the N + 1 descending times of N user steps -> the program (module docstring).
    `eta` in [0, 1] (how much of each step's noise is re-drawn) and `s_noise` >= 0 (a factor on the drawn noise) shape the stochastic
    samplers alone; a deterministic one ignores them."""
    if name not in SAMPLERS + STOCHASTIC_SAMPLERS:
        raise ValueError(f"fluxmi: sampler={name!r}: expected one of {SAMPLERS + STOCHASTIC_SAMPLERS}")
    try:
        eta, s_noise = float(eta), float(s_noise)
    except (TypeError, ValueError):
        raise ValueError(f"fluxmi: eta={eta!r}, s_noise={s_noise!r}: expected numbers") from None
    if not 0.0 <= eta <= 1.0:  # (NaN fails both)
        raise ValueError(f"fluxmi: eta={eta}: expected a value in [0, 1]")
    if not (math.isfinite(s_noise) and s_noise >= 0.0):
        raise ValueError(f"fluxmi: s_noise={s_noise}: expected a finite value >= 0")
    s = check_sigmas(sigmas)
    if name in STOCHASTIC_SAMPLERS and s[0] > 1.0:
        raise ValueError(f"fluxmi: sampler={name!r} needs sigmas in (0, 1] (alpha = 1 - sigma), got {s[0]}")
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
        elif name == "euler_ancestral":
            sd = b * (1.0 + (b / a - 1.0) * eta)
            r, k = sd / a, (1.0 - b) / (1.0 - sd)
            cn = s_noise * math.sqrt(max(0.0, b * b - (sd * k) ** 2))  # (eta = 0: k is 1.0 and sd is b exactly, so cn is 0 exactly)
            emit(a, _row(cx=k * r, ga=1.0, gb=-a, c0=k * (1.0 - r), cn=cn), _ctl(), i)
        elif name == "dpmpp_2m_sde":
            E = (b / a) * ((1.0 - a) / (1.0 - b))
            cD = (1.0 - b) * (1.0 - E ** (1.0 + eta))
            row = dict(cx=(b / a) * E ** eta, ga=1.0, gb=-a, cn=s_noise * b * math.sqrt(max(0.0, 1.0 - E ** (2.0 * eta))))
            w_slot = -1 if last else i % 2
            if i == 0 or s[i - 1] == 1.0:  # no history, or one whose log-SNR step is infinite
                emit(a, _row(c0=cD, **row), _ctl(w_slot=w_slot), i)
            else:
                lam = lambda v: math.log((1.0 - v) / v)
                r = (lam(a) - lam(s[i - 1])) / (lam(b) - lam(a))
                c1 = -cD / (2.0 * r)
                emit(a, _row(c0=cD - c1, c1=c1, **row), _ctl(w_slot=w_slot, h1_slot=(i - 1) % 2), i)
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
