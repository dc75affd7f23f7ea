"""Request traces: caller-supplied traffic for a batched handle (include/orlg.h ``orlg_trace``).

A generated handle draws its requests on the device (MT19937, ``expovariate``, ``choices`` / ``randint``).  A trace handle
replays a recorded or synthetic sequence instead: environment ``i`` serves request 0, 1, 2, ... of row ``i``; everything
else of the step is unchanged.  A trace of ``n`` requests per environment allows ``n - 1`` steps after a full reset (the
reset draws request 0, every step draws the next one).

Everything in this module is host arithmetic: importable and testable without a device or the library.  The checks are the
library's own (``orlg_create_trace``), so a trace this module accepts is one the library accepts for a matching handle.
"""
from __future__ import annotations

import ctypes as C
import heapq

import numpy as np

from . import traffic as _traffic

FIELDS = ("arrival", "holding", "src", "dst", "bit_rate")


class TraceError(ValueError):
    """A trace entry breaks a rule; ``env`` and ``index`` name it (``None`` for a rule about the whole trace)."""

    def __init__(self, msg, env=None, index=None):
        where = "" if env is None else f"environment {env}, request {index}: "
        super().__init__(f"trace: {where}{msg}")
        self.env, self.index = env, index


def _env_major(name, a, dtype, batch_size, length, layout):
    a = np.asarray(a)
    if dtype == np.int32:
        if a.dtype.kind not in "iu":
            raise TypeError(f"{name}: dtype {a.dtype}, expected an integer type")
    elif a.dtype.kind not in "fiu":
        raise TypeError(f"{name}: dtype {a.dtype}, expected a real type")
    if a.ndim == 1:
        if a.shape != (length,):
            raise TraceError(f"{name}: shape {a.shape}, expected ({length},)")
        a = np.broadcast_to(a, (batch_size, length))
    elif a.ndim == 2:
        want = (length, batch_size) if layout == "step" else (batch_size, length)
        if a.shape != want:
            raise TraceError(f"{name}: shape {a.shape}, expected {want} ({layout}-major) or ({length},)")
        if layout == "step":
            a = a.T
    else:
        raise TraceError(f"{name}: {a.ndim} dimensions, expected [n], [n][B] (step-major) or [B][n] (env-major)")
    return np.ascontiguousarray(a, dtype=dtype)


class RequestTrace:
    """``n`` requests for each of ``B`` environments.

    ``arrival`` (absolute arrival time) and ``holding`` are float64, ``src`` / ``dst`` / ``bit_rate`` int32 (the rate's
    value, not an index).  Every array is ``[n][B]`` step-major -- what ``run(outputs=...)`` returns -- or ``[B][n]``
    env-major, or ``[n]`` for one sequence every environment replays; ``layout`` says which of the two 2-D layouts is meant
    (``"auto"``: step-major unless only the env-major reading fits ``batch_size``).  The arrays are kept env-major.

    The rules checked here without a topology: shapes agree, ``n >= 2``, times finite, arrivals >= 0 and non-decreasing per
    environment, holdings >= 0, ``src != dst`` and both >= 0.  ``validate(...)`` adds what depends on the handle: nodes
    below ``num_nodes``, rates in the table or inside the continuous bounds.
    """

    def __init__(self, arrival, holding, src, dst, bit_rate, *, batch_size=None, layout="auto"):
        if layout not in ("auto", "step", "env"):
            raise ValueError("layout must be 'auto', 'step' or 'env'")
        arrays = [np.asarray(x) for x in (arrival, holding, src, dst, bit_rate)]
        two_d = [x for x in arrays if x.ndim == 2]
        if any(x.ndim not in (1, 2) for x in arrays):
            raise TraceError("every array is [n], [n][B] (step-major) or [B][n] (env-major)")
        if two_d:
            first = two_d[0]
            if layout == "auto":
                layout = "step"
                if batch_size is not None and first.shape[1] != int(batch_size) and first.shape[0] == int(batch_size):
                    layout = "env"
            length, B = (first.shape[0], first.shape[1]) if layout == "step" else (first.shape[1], first.shape[0])
            if batch_size is not None and int(batch_size) != B:
                raise TraceError(f"shape {first.shape} does not fit batch_size {batch_size}")
        else:
            length, B = arrays[0].shape[0], 1 if batch_size is None else int(batch_size)
            layout = "step"
        if B < 1:
            raise TraceError("batch_size must be >= 1")
        self.batch_size, self.length = int(B), int(length)
        self.arrival = _env_major("arrival", arrival, np.float64, B, length, layout)
        self.holding = _env_major("holding", holding, np.float64, B, length, layout)
        self.src = _env_major("src", src, np.int32, B, length, layout)
        self.dst = _env_major("dst", dst, np.int32, B, length, layout)
        self.bit_rate = _env_major("bit_rate", bit_rate, np.int32, B, length, layout)
        self.validate()

    # ------------------------------------------------------------------ rules
    @staticmethod
    def _first(bad):
        i, j = np.argwhere(bad)[0]
        return int(i), int(j)

    def validate(self, num_nodes=None, bit_rates=None, bit_rate_bounds=None):
        """Raise :class:`TraceError` naming the first offending (environment, index).  ``bit_rates``: the table of a
        discrete handle; ``bit_rate_bounds``: (lower, higher) of a continuous one."""
        if self.length < 2:
            raise TraceError(f"length {self.length}: a trace has at least 2 requests per environment")
        a, h = self.arrival, self.holding
        bad = ~np.isfinite(a) | (a < 0)
        if bad.any():
            i, j = self._first(bad)
            raise TraceError(f"arrival {a[i, j]} is not a finite time >= 0", i, j)
        bad = np.zeros(a.shape, bool)
        bad[:, 1:] = a[:, 1:] < a[:, :-1]
        if bad.any():
            i, j = self._first(bad)
            raise TraceError(f"arrival {a[i, j]!r} before its predecessor's {a[i, j - 1]!r}", i, j)
        bad = ~np.isfinite(h) | (h < 0)
        if bad.any():
            i, j = self._first(bad)
            raise TraceError(f"holding {h[i, j]} is not a finite time >= 0", i, j)
        hi = np.iinfo(np.int32).max if num_nodes is None else int(num_nodes) - 1
        bad = (self.src < 0) | (self.dst < 0) | (self.src > hi) | (self.dst > hi)
        if bad.any():
            i, j = self._first(bad)
            raise TraceError(f"node pair ({self.src[i, j]}, {self.dst[i, j]}) outside 0..{hi}", i, j)
        bad = self.src == self.dst
        if bad.any():
            i, j = self._first(bad)
            raise TraceError(f"source and destination are both {self.src[i, j]}", i, j)
        if bit_rates is not None:
            bad = ~np.isin(self.bit_rate, np.asarray(bit_rates, np.int64))
            if bad.any():
                i, j = self._first(bad)
                raise TraceError(f"bit rate {self.bit_rate[i, j]} is not one of the handle's bit rates", i, j)
        if bit_rate_bounds is not None:
            lo, up = bit_rate_bounds
            bad = (self.bit_rate < lo) | (self.bit_rate > up)
            if bad.any():
                i, j = self._first(bad)
                raise TraceError(f"bit rate {self.bit_rate[i, j]} outside the bounds {lo}..{up}", i, j)
        return self

    # ------------------------------------------------------------------ what the capacities are sized from
    def peak_offered(self) -> int:
        """The largest number of requests simultaneously inside ``[arrival, arrival + holding]`` (closed) over all
        environments: an upper bound on the running services of any policy, and what a trace handle sizes its release queue
        from (``queue_capacity=0``)."""
        peak = 0
        for i in range(self.batch_size):
            ends = []
            for a, h in zip(self.arrival[i].tolist(), self.holding[i].tolist()):
                while ends and ends[0] < a:
                    heapq.heappop(ends)
                heapq.heappush(ends, a + h)
                peak = max(peak, len(ends))
        return peak

    # ------------------------------------------------------------------ plumbing
    def __eq__(self, other):
        return isinstance(other, RequestTrace) and all(
            np.array_equal(getattr(self, f), getattr(other, f)) for f in FIELDS)

    __hash__ = None

    def __repr__(self):
        return f"RequestTrace(batch_size={self.batch_size}, length={self.length})"

    def for_batch(self, batch_size):
        """This trace for a handle of ``batch_size`` environments: itself when it fits, one sequence broadcast otherwise."""
        if self.batch_size == int(batch_size):
            return self
        if self.batch_size != 1:
            raise TraceError(f"{self.batch_size} environments, the handle has {batch_size}")
        return RequestTrace(*(getattr(self, f)[0] for f in FIELDS), batch_size=batch_size)

    def struct(self, groups=None, num_groups=1):
        """The ``orlg_trace`` of a handle (the arrays stay referenced by this object)."""
        from . import _lib
        t = _lib.Trace()
        t.length = self.length
        for f in FIELDS:
            setattr(t, f, getattr(self, f).ctypes.data_as(C.c_void_p))
        self._groups = None if groups is None else np.ascontiguousarray(groups, np.int32)
        t.group = None if groups is None else self._groups.ctypes.data_as(C.c_void_p)
        t.num_groups = int(num_groups)
        return t

    @classmethod
    def from_golden(cls, z, batch_size=None):
        """The request stream of a golden file of tests/golden (``src_id, dst_id, bit_rate, arrival, holding`` per step)."""
        return cls(z["arrival"], z["holding"], z["src_id"], z["dst_id"], z["bit_rate"], batch_size=batch_size)


def check_trace_kwargs(trace, given):
    """``trace=`` excludes the arguments that describe generated traffic; ``given``: name -> value as the caller passed them
    (``None`` = not passed)."""
    if trace is None:
        return
    if not isinstance(trace, RequestTrace):
        raise TypeError("trace: a RequestTrace")
    clash = [k for k, v in given.items() if v is not None]
    if clash:
        raise ValueError(f"trace= replays recorded requests: {', '.join(sorted(clash))} describe generated traffic and cannot be "
                         "passed with it")


def trace_groups(batch_size, groups, num_groups):
    return _traffic.check_groups(batch_size, groups, num_groups)


def record_trace(env, policy, n_steps, **run_kwargs):
    """Run ``policy`` for ``n_steps`` on a batched handle and return the ``n_steps + 1`` requests per environment it saw: the
    served ones from the step outputs plus the pending one from ``requests()``.  ``trace.outputs`` keeps what ``env.run``
    returned (the caller's ``outputs=`` plus request / arrival / holding)."""
    want = list(run_kwargs.pop("outputs", ()))
    names = want + [n for n in ("request", "arrival", "holding") if n not in want]
    res = env.run(policy, int(n_steps), outputs=names, **run_kwargs)
    pend = env.requests()
    req = res["request"]
    arrival = np.concatenate([res["arrival"], pend["arrival_time"][None, :]])
    holding = np.concatenate([res["holding"], pend["holding_time"][None, :]])
    src = np.concatenate([req[:, :, 1], pend["src"][None, :]])
    dst = np.concatenate([req[:, :, 2], pend["dst"][None, :]])
    rate = np.concatenate([req[:, :, 3], pend["bit_rate"][None, :]])
    trace = RequestTrace(arrival, holding, src, dst, rate, batch_size=env.batch_size, layout="step")
    trace.outputs = res
    return trace
