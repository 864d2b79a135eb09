"""Weighted 1-D Wasserstein distances between observable distributions and fixed reference distributions
(mythos/observables/wasserstein.py:14-149), evaluated by the HIP library (mythos_amd/csrc/w1.hip).

    wd = WassersteinDistanceMapped(observable=BondDistancesMapped(topology=top, bond_names=names),
                                   v_distribution_map={name: reference_samples, ...})
    per_name = wd(trajectory, weights)        # {name: 0-dim float64 device tensor}, differentiable in ``weights``

The reference sorts the samples three times per name on every call and differentiates through the sorts.  Inside a
DiffTRe optimisation the samples of a stored trajectory do not change between optimisation steps, only the frame
weights do, so here the merged order is computed once (a *plan*: one stable sort per name) and every later call is a
gather of the weights, a prefix sum and - for the gradient - a suffix sum, a fixed handful of launches for all names
together - per ``WassersteinDistance*`` object: a loss that holds bonds and angles in two objects runs the set twice -
with the analytic dW/dweights (sign(0) = 0 where the reference differentiates ``jnp.abs``).

What is cached, and when it is dropped: a ``WassersteinDistance*`` object holds at most ONE plan.  The key is the
content of the observable's sample block, not the identity of the trajectory tensors (``DiffTReObjective.calculate``
concatenates its trajectories anew on every step): every call evaluates the observable (one cheap launch for the
MARTINI geometry classes) and compares the block bit for bit, on the device, with the block the plan was built from;
equal means reuse.  The plan keeps that block and its own arrays and no trajectory alive; a miss replaces it,
``release()`` drops it.  A call on the reuse path does one device-to-host read (the comparison and the mass check
together) however many keys it has; building a plan adds the sorts and one more synchronisation.

Gradients with respect to the sample values are not provided (DiffTRe never asks for them): samples that require
grad raise ``ValueError``.  Reference weights are masses (>= 0).
"""

from __future__ import annotations

import ctypes as C
import dataclasses as dc
import math
from typing import Any

import numpy as np
import torch

from mythos_amd import _lib

_PLANS_BUILT = 0


def plans_built() -> int:
    """Plans built so far in this process (tests and diagnostics: a reused plan does not count)."""
    return _PLANS_BUILT


def _as_f64(x, device=None) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    return t.detach().to(dtype=torch.float64, device=device if device is not None else t.device)


def _check_shapes(u_shape, v_shape, u_weights_shape, v_weights_shape) -> None:
    """The two shape errors of wasserstein.py:29-33 (host only)."""
    if u_weights_shape is not None and tuple(u_weights_shape) != tuple(u_shape):
        raise ValueError(f"u_weights must have the same shape as u; got {tuple(u_weights_shape)} and {tuple(u_shape)}.")
    if v_weights_shape is not None and tuple(v_weights_shape) != tuple(v_shape):
        raise ValueError(f"v_weights must have the same shape as v; got {tuple(v_weights_shape)} and {tuple(v_shape)}.")


def _check_mass(sum_u: float, sum_v: float) -> None:
    """wasserstein.py:36-40 (jnp.isclose(rtol=1e-5, atol=1e-5))."""
    if not abs(sum_u - sum_v) <= 1e-5 + 1e-5 * abs(sum_v):
        raise ValueError(f"u_weights and v_weights must sum to the same total mass; got {sum_u} and {sum_v}.")


class W1Plan(_lib.Handle):
    """mythos_w1_plan_t plus the sample block it was built from.  ``values``: per group a float64 device tensor
    whose first axis is the frame axis; ``refs`` / ``ref_weights``: per group a flat float64 device tensor (weights
    may be None)."""

    _destroy = "mythos_w1_plan_destroy"

    def __init__(self, block: torch.Tensor, frames: list, members: list, refs: list, ref_weights: list):
        global _PLANS_BUILT
        self.device = block.device
        self.block, self.frames, self.members = block, list(frames), list(members)
        self.n_groups, self.max_frames = len(frames), max(frames)
        orders, at = [], 0
        for s, m, v in zip(frames, members, refs):
            u = block[at:at + s * m]
            at += s * m
            orders.append(torch.sort(torch.cat([u, v]), stable=True).indices)
        order = torch.cat(orders).contiguous()
        ref = torch.cat(refs).contiguous()
        has = np.ascontiguousarray([w is not None for w in ref_weights], dtype=np.uint8)
        vw = None
        if has.any():
            vw = torch.cat([w if w is not None else torch.zeros_like(v) for w, v in zip(ref_weights, refs)]).contiguous()
        fr = np.ascontiguousarray(frames, dtype=np.int32)
        mem = np.ascontiguousarray(members, dtype=np.int32)
        nref = np.ascontiguousarray([int(v.numel()) for v in refs], dtype=np.int64)
        super().__init__(
            "mythos_w1_plan_create", self.n_groups, fr.ctypes.data_as(_lib.c_int_p), mem.ctypes.data_as(_lib.c_int_p), _lib.ptr(block),
            nref.ctypes.data_as(C.POINTER(C.c_int64)), _lib.ptr(ref), _lib.ptr(vw),
            has.ctypes.data_as(_lib.c_uint8_p) if vw is not None else None, _lib.ptr(order), self.device.index or 0,
            _lib.stream(self.device))
        _PLANS_BUILT += 1

    def close(self):
        super().close()
        self.block = None

    def same_block(self, block, frames, members) -> torch.Tensor | None:
        """Device bool: ``block`` equals, bit for bit, the block this plan was built from (None: another layout)."""
        if self.block is None or list(frames) != self.frames or list(members) != self.members or block.device != self.device:
            return None
        return (block.view(torch.int64) == self.block.view(torch.int64)).all()

    def eval(self, weights: torch.Tensor | None, want_grad: bool):
        """(w1 (G,), dw1/dweights (G, max frames) or None) for float64 device weights (S,) or None."""
        w1 = torch.empty(self.n_groups, dtype=torch.float64, device=self.device)
        dw = torch.zeros((self.n_groups, self.max_frames), dtype=torch.float64, device=self.device) if want_grad else None
        _lib.check(self._lib.mythos_w1_eval(self._h, _lib.ptr(weights), _lib.ptr(w1), _lib.ptr(dw), _lib.stream(self.device)), "w1_eval")
        return w1, dw


class _W1Op(torch.autograd.Function):
    """W of every group as a function of the frame weights; backward = the kernel's dW/dweights contracted with the
    incoming gradient."""

    @staticmethod
    def forward(ctx, weights, plan):
        w1, dw = plan.eval(weights.detach().contiguous(), ctx.needs_input_grad[0])
        ctx.save_for_backward(*([dw] if dw is not None else []))
        return w1

    @staticmethod
    def backward(ctx, g_out):
        (dw,) = ctx.saved_tensors
        return (g_out.to(dw.dtype)[:, None] * dw).sum(0), None


def _need_gpu(t: torch.Tensor) -> None:
    if t.device.type != "cuda":
        raise _lib.MythosHipError("Wasserstein distances are evaluated by the HIP library: the samples must live on a GPU "
                                  "(mythos_amd has no CPU fallback)")


def _run(plan: W1Plan, weights: torch.Tensor | None) -> torch.Tensor:
    if weights is None:
        return plan.eval(None, False)[0]
    return _W1Op.apply(weights.to(device=plan.device, dtype=torch.float64), plan)


def wasserstein_1d(u, v, u_weights=None, v_weights=None) -> torch.Tensor:
    """1-D Wasserstein distance between the weighted samples u and v (wasserstein.py:14-63) as a 0-dim float64 device
    tensor, differentiable in ``u_weights``.  The argument errors are raised before any device work."""
    if isinstance(u, torch.Tensor) and u.requires_grad:
        raise ValueError("gradients with respect to the sample values are not provided")
    u, v = _as_f64(u), _as_f64(v)
    uw = None if u_weights is None else (u_weights if isinstance(u_weights, torch.Tensor) else torch.as_tensor(np.asarray(u_weights)))
    vw = None if v_weights is None else _as_f64(v_weights)
    _check_shapes(u.shape, v.shape, None if uw is None else uw.shape, None if vw is None else vw.shape)
    if vw is not None and bool((vw < 0).any()):
        raise ValueError("v_weights are masses: negative values are not accepted")
    _check_mass(1.0 if uw is None else float(uw.detach().double().sum()), 1.0 if vw is None else float(vw.sum()))
    device = u.device if u.device.type == "cuda" else (torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else u.device)
    u = u.to(device).reshape(-1).contiguous()
    _need_gpu(u)
    plan = W1Plan(u, [int(u.numel())], [1], [v.to(device).reshape(-1)], [None if vw is None else vw.to(device).reshape(-1)])
    try:
        return _run(plan, None if uw is None else uw.reshape(-1))[0]
    finally:
        plan.close()


class _Cached:
    """One plan per object, keyed by the content of the sample block."""

    def release(self) -> None:
        """Drop the cached plan (its device arrays and the sample block it holds)."""
        plan = self.__dict__.pop("_plan", None)
        if plan is not None:
            plan.close()

    def _refs(self, keys, v_map, vw_map, device):
        """Reference samples and weights on the device (flat float64), their masses on the host; cached per device."""
        cache = self.__dict__.setdefault("_ref_cache", {})
        if str(device) not in cache:
            refs = [_as_f64(v_map[k], device).reshape(-1).contiguous() for k in keys]
            vws = [None if vw_map.get(k) is None else _as_f64(vw_map[k], device).reshape(-1).contiguous() for k in keys]
            if any(w is not None and bool((w < 0).any()) for w in vws):
                raise ValueError("v_weights are masses: negative values are not accepted")
            masses = [1.0 if w is None else float(w.sum()) for w in vws]
            cache[str(device)] = (refs, vws, masses)
        return cache[str(device)]

    def _evaluate(self, keys, values, packed, v_map, vw_map, weights) -> torch.Tensor:
        """W per key (G,) for per-key sample tensors ``values`` (first axis: frames) or an already packed block."""
        for k in keys:  # host-side argument checks first
            vw = vw_map.get(k)
            if vw is not None:
                _check_shapes((), np.shape(v_map[k]), None, np.shape(vw))
        if packed is not None:
            block, s, mem = packed
            if len(mem) != len(keys):
                raise ValueError(f"the observable returns {len(mem)} groups of values for {len(keys)} reference distribution(s): "
                                 "use WassersteinDistanceMapped for a *Mapped observable with several names")
            frames, members = [s] * len(mem), list(mem)
        else:
            frames, members = [], []
            for k, val in zip(keys, values):
                if not isinstance(val, torch.Tensor):
                    raise TypeError(f"observable value for '{k}' is not a torch tensor")
                if val.requires_grad:
                    raise ValueError("gradients with respect to the sample values are not provided: detach the observable")
                _need_gpu(val)
                frames.append(int(val.shape[0]) if val.dim() > 0 else 1)
                members.append(max(1, math.prod(val.shape[1:])) if val.dim() > 0 else 1)
            block = torch.cat([val.detach().to(torch.float64).reshape(-1) for val in values]).contiguous()
        if weights is not None:
            weights = weights if isinstance(weights, torch.Tensor) else torch.as_tensor(np.asarray(weights))
            for s, m in zip(frames, members):
                if weights.dim() != 1 or int(weights.shape[0]) != s:
                    n = int(weights.numel())
                    _check_shapes((s * m,), (), (n * m,), None)
            weights = weights.to(device=block.device, dtype=torch.float64)
        refs, vws, masses = self._refs(keys, v_map, vw_map, block.device)
        plan = self.__dict__.get("_plan")
        same = None if plan is None else plan.same_block(block, frames, members)
        # one read: [block unchanged, sum of the frame weights]
        head = torch.stack([torch.ones((), dtype=torch.float64, device=block.device) if same is None else same.to(torch.float64),
                            torch.ones((), dtype=torch.float64, device=block.device) if weights is None else weights.detach().sum()]).cpu()
        for mass in masses:
            _check_mass(float(head[1]), mass)
        if same is None or float(head[0]) == 0.0:
            self.release()
            plan = W1Plan(block, frames, members, refs, vws)
            self.__dict__["_plan"] = plan
        return _run(plan, weights)


@dc.dataclass(frozen=True, kw_only=True)
class WassersteinDistance(_Cached):
    """W between the distribution of ``observable(trajectory)`` ((S, n_values), flattened) and ``v_distribution``
    (wasserstein.py:81-111).  ``weights`` at call time are per frame and apply to all values of that frame."""

    observable: Any
    v_distribution: Any
    v_weights: Any = None

    def __call__(self, trajectory, weights=None) -> torch.Tensor:
        packed = None
        fast = getattr(self.observable, "packed", None)
        values = None
        if fast is not None:
            packed = fast(trajectory)
        else:
            values = [self.observable(trajectory)]
        return self._evaluate(["v"], values, packed, {"v": self.v_distribution}, {"v": self.v_weights}, weights)[0]


@dc.dataclass(frozen=True, kw_only=True)
class WassersteinDistanceMapped(_Cached):
    """The same by key (wasserstein.py:114-149): ``observable`` returns a dict, the output keys are exactly those of
    ``v_distribution_map``; a key missing from ``v_weights_map`` means uniform reference weights."""

    observable: Any
    v_distribution_map: dict
    v_weights_map: dict = dc.field(default_factory=dict)

    def __call__(self, trajectory, weights=None) -> dict:
        keys = list(self.v_distribution_map)
        packed, values = None, None
        fast = getattr(self.observable, "packed", None)
        if fast is not None and tuple(getattr(self.observable, "names", ())) == tuple(keys):
            packed = fast(trajectory)
        else:
            obs = self.observable(trajectory)
            values = [obs[k] for k in keys]
        w = self._evaluate(keys, values, packed, self.v_distribution_map, self.v_weights_map, weights)
        return {k: w[i] for i, k in enumerate(keys)}
