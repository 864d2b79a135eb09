"""Thin object wrappers over the C ABI handles (device memory is owned by torch tensors).

``OxdnaSystem``  <-> mythos_system_t   (topology + parameters + neighbour rows)
``LangevinIntegrator`` <-> mythos_sim_t

These are plumbing: they validate shapes/dtypes/devices and forward pointers.  The reference-
shaped API (EnergyFunction / Simulator protocols) lives in ``mythos_amd.energy`` and
``mythos_amd.simulators`` on top of them.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from mythos_amd import _lib

N_TERMS = 8
TRACE_WIDTH = 10
TERM_NAMES = (
    "fene",
    "bonded_excluded_volume",
    "stacking",
    "unbonded_excluded_volume",
    "hydrogen_bonding",
    "cross_stacking",
    "coaxial_stacking",
    "debye",
)


class OxdnaSystem(_lib.Handle):
    """One oxDNA system on one GPU."""

    _destroy = "mythos_oxdna_destroy"

    def __init__(self, model: int, seq, is_end, bonded, box=None, dtype=torch.float32, device=None, is_rna=None):
        if _lib.device_count() == 0 or not torch.cuda.is_available():
            raise _lib.MythosHipError("no HIP device visible: the mythos_amd HIP path has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("OxdnaSystem needs a cuda (HIP) device")
        self.dtype = dtype
        self.model = int(model)
        seq = np.ascontiguousarray(seq, dtype=np.int32)
        self.n = int(seq.shape[0])
        is_end = np.zeros(self.n, np.uint8) if is_end is None else np.ascontiguousarray(is_end, dtype=np.uint8)
        bonded = np.ascontiguousarray(bonded, dtype=np.int32).reshape(-1, 2)
        box_arr = None if box is None else np.ascontiguousarray(np.broadcast_to(np.asarray(box, np.float64), (3,)))
        self.box = box_arr
        super().__init__(
            "mythos_oxdna_create",
            self.model,
            self.n,
            seq.ctypes.data_as(_lib.c_int_p),
            is_end.ctypes.data_as(_lib.c_uint8_p),
            int(bonded.shape[0]),
            bonded.ctypes.data_as(_lib.c_int_p),
            None if box_arr is None else box_arr.ctypes.data_as(_lib.c_double_p),
            _lib.dtype_code(dtype),
            self.device.index or 0,
        )
        self._pseq_n_bp = 0
        self._pseq_terms = 0
        self._op_lists = None  # (ops, kind, first, pairs) of the last order_params call
        # oxNA (model 4): three vectors - oxDNA2, oxRNA2, hybrid - one after the other; dU/dparams rows likewise
        self.n_params = self._lib.mythos_oxdna_param_count() * (3 if self.model == 4 else 1)
        if self.model == 4:
            if is_rna is None:
                raise ValueError("an oxNA system (model 4) needs is_rna, the type of every nucleotide")
            t = np.ascontiguousarray(is_rna, dtype=np.uint8)
            if t.shape != (self.n,):
                raise ValueError(f"is_rna must have shape ({self.n},)")
            _lib.check(self._lib.mythos_oxdna_set_nucleotide_types(self._h, t.ctypes.data_as(_lib.c_uint8_p)), "set_nucleotide_types")

    # ---- parameters / neighbours -------------------------------------------------------------
    def set_params(self, flat) -> None:
        flat = np.ascontiguousarray(torch.as_tensor(flat).detach().cpu().numpy(), dtype=np.float64)
        _lib.check(
            self._lib.mythos_oxdna_set_params(self._h, flat.ctypes.data_as(_lib.c_double_p), int(flat.shape[0])),
            "set_params",
        )

    def set_pseq(self, marginals=None, unit=None, bp_probs=None, terms: int = 0) -> None:
        """Probabilistic sequence (mythos_oxdna_set_pseq); ``terms`` = 0 or no arguments: back to the discrete sequence."""
        if not terms:
            _lib.check(self._lib.mythos_oxdna_set_pseq(self._h, None, None, 0, None, 0), "set_pseq")
            self._pseq_terms = 0
            return
        marg = np.ascontiguousarray(marginals, dtype=np.float64)
        unit = np.ascontiguousarray(unit, dtype=np.int32)
        bp = np.ascontiguousarray(bp_probs, dtype=np.float64).reshape(-1, 4)
        if marg.shape != (self.n, 4) or unit.shape != (self.n,):
            raise ValueError(f"marginals must be ({self.n}, 4) and unit ({self.n},)")
        # every row of bp_probs is a constrained base pair (the library checks that unit names each of them exactly
        # twice, once per member); a system without base pairs passes one row of zeros, as the reference does
        n_bp = int(bp.shape[0]) if (unit >= 0).any() else 0
        self._pseq_n_bp = n_bp
        if (unit >= 0).any() and int(unit.max()) >= 2 * n_bp:
            raise ValueError("bp_probs has fewer rows than the base pairs named in unit")
        _lib.check(self._lib.mythos_oxdna_set_pseq(self._h, marg.ctypes.data_as(_lib.c_double_p), unit.ctypes.data_as(_lib.c_int_p),
                                                   n_bp, bp.ctypes.data_as(_lib.c_double_p), int(terms)), "set_pseq")
        self._pseq_terms = int(terms)

    def set_neighbors(self, pairs) -> None:
        pairs = np.ascontiguousarray(pairs, dtype=np.int32)
        if pairs.ndim != 2 or (pairs.size and pairs.shape[1] != 2):
            raise ValueError("pairs must have shape (P, 2)")
        _lib.check(
            self._lib.mythos_oxdna_set_neighbors(self._h, pairs.ctypes.data_as(_lib.c_int_p), int(pairs.shape[0])),
            "set_neighbors",
        )

    def build_neighbors(self, center: torch.Tensor, r_cut: float, skin: float) -> None:
        c = self._check(center, (self.n, 3), "center")
        _lib.check(
            self._lib.mythos_oxdna_build_neighbors(self._h, _lib.ptr(c), float(r_cut), float(skin), _lib.stream(self.device)),
            "build_neighbors",
        )

    def neighbor_stats(self) -> tuple[int, float]:
        mx, mean = C.c_int(0), C.c_double(0.0)
        _lib.check(self._lib.mythos_oxdna_neighbor_stats(self._h, C.byref(mx), C.byref(mean)), "neighbor_stats")
        return mx.value, mean.value

    def rows(self):
        """(rows (n, stride) int32, len (n,) int32, close (n,) int32) of the neighbour rows the device holds, as numpy
        arrays: row i is its bonded slots, then the close segment [bonded slots, close[i]), then the far segment
        [close[i], len[i]); an entry is neighbour index | role bit (diagnostics / tests; synchronises)."""
        stride = C.c_int(0)
        _lib.check(self._lib.mythos_oxdna_get_rows(self._h, None, None, None, C.byref(stride)), "get_rows")
        rows = np.empty((self.n, stride.value), dtype=np.int32)
        lens = np.empty(self.n, dtype=np.int32)
        close = np.empty(self.n, dtype=np.int32)
        p32 = C.POINTER(C.c_int32)
        _lib.check(self._lib.mythos_oxdna_get_rows(self._h, rows.ctypes.data_as(p32), lens.ctypes.data_as(p32),
                                                   close.ctypes.data_as(p32), C.byref(stride)), "get_rows")
        return rows, lens, close

    # ---- energy --------------------------------------------------------------------------------
    def _check(self, t: torch.Tensor, tail: tuple, name: str) -> torch.Tensor:
        if not isinstance(t, torch.Tensor) or t.device != self.device:
            raise ValueError(f"{name} must be a torch tensor on {self.device}")
        if t.dtype != self.dtype:
            raise ValueError(f"{name} must have dtype {self.dtype}, got {t.dtype}")
        if tuple(t.shape[-len(tail):]) != tail:
            raise ValueError(f"{name} must have trailing shape {tail}, got {tuple(t.shape)}")
        return t.contiguous()

    def _frames(self, center, quat):
        """center (F, N, 3) or (N, 3), quat likewise with 4 -> (contiguous (F, N, 3), (F, N, 4), F, whether it was one frame)."""
        single = center.dim() == 2
        c = self._check(center, (self.n, 3), "center")
        q = self._check(quat, (self.n, 4), "quat")
        if single:
            c, q = c[None], q[None]
        if q.shape[0] != c.shape[0]:
            raise ValueError("center and quat disagree on the number of frames")
        return c, q, int(c.shape[0]), single

    def energy(self, center, quat, *, grads=False, param_grads=False, observables=None, pseq_grads=False):
        """Term energies (F, 8) [float64] and optionally dU/dcenter, dU/dquat, dU/dflat.

        ``center`` (F, N, 3) or (N, 3); ``quat`` likewise with 4.  ``observables``: an
        ``mythos_amd.observables.ObservableSet`` evaluated in the same call (the observables kernel queued right behind the energy launch); its (F, width) rows are
        then returned as a fifth value.  ``pseq_grads`` (with ``param_grads``, after ``set_pseq``): also
        dU/d(marginals) (F, N, 4) and dU/d(base-pair type probabilities) (F, max(n_bp, 1), 4), as a fifth and sixth value.
        """
        c, q, nf, single = self._frames(center, quat)
        e = torch.empty((nf, N_TERMS), dtype=torch.float64, device=self.device)
        gc = torch.empty_like(c) if grads else None
        gq = torch.empty_like(q) if grads else None
        gp = torch.empty((nf, self.n_params), dtype=torch.float64, device=self.device) if param_grads else None
        if pseq_grads:
            if not param_grads or observables is not None:
                raise ValueError("pseq_grads comes with param_grads and without fused observables")
            gm = torch.empty((nf, self.n, 4), dtype=torch.float64, device=self.device)
            gb = torch.empty((nf, max(self._pseq_n_bp, 1), 4), dtype=torch.float64, device=self.device)
            _lib.check(
                self._lib.mythos_oxdna_energy_dpseq(
                    self._h, _lib.ptr(c), _lib.ptr(q), nf, _lib.ptr(e), _lib.ptr(gc), _lib.ptr(gq), _lib.ptr(gp), _lib.ptr(gm),
                    _lib.ptr(gb), _lib.stream(self.device),
                ),
                "energy_dpseq",
            )
            if single:
                return e[0], (gc[0] if grads else None), (gq[0] if grads else None), gp[0], gm[0], gb[0]
            return e, gc, gq, gp, gm, gb
        if observables is not None and not getattr(observables, "fusable", True):
            raise ValueError(f"{type(observables).__name__} is not evaluated in the energy call (the fused energy + observables "
                             "path takes an ObservableSet of propeller twist / rise / pitch / persistence length)")
        if observables is None:
            _lib.check(
                self._lib.mythos_oxdna_energy(
                    self._h, _lib.ptr(c), _lib.ptr(q), nf, _lib.ptr(e), _lib.ptr(gc), _lib.ptr(gq), _lib.ptr(gp),
                    _lib.stream(self.device),
                ),
                "energy",
            )
            rows = None
        else:
            rows = torch.empty((nf, observables.width), dtype=torch.float64, device=self.device)
            _lib.check(
                self._lib.mythos_oxdna_energy_obs(
                    self._h, _lib.ptr(c), _lib.ptr(q), nf, _lib.ptr(e), _lib.ptr(gc), _lib.ptr(gq), _lib.ptr(gp),
                    observables._h, _lib.ptr(rows), _lib.stream(self.device),
                ),
                "energy_obs",
            )
        if single:
            e = e[0]
            gc = gc[0] if grads else None
            gq = gq[0] if grads else None
            gp = gp[0] if param_grads else None
        if observables is not None:
            return e, gc, gq, gp, rows
        return e, gc, gq, gp


    def debye_sweep(self, center, quat, table, *, const_grads=False):
        """Debye-Hueckel energy of every frame at every row of ``table`` (T, 5) [kappa, prefactor, bsmooth, rcut, rhigh]
        (mythos_oxdna_debye_sweep): (e_dh (T, F) float64, de/dconstants (T, F, 5) or None).  oxDNA2 and oxRNA2 systems."""
        c, q, nf, _ = self._frames(center, quat)
        table = np.ascontiguousarray(table, dtype=np.float64)
        if table.ndim != 2 or table.shape[1] != 5:
            raise ValueError("table must have shape (T, 5)")
        nt = int(table.shape[0])
        e = torch.empty((nt, nf), dtype=torch.float64, device=self.device)
        de = torch.empty((nt, nf, 5), dtype=torch.float64, device=self.device) if const_grads else None
        self._sweep_table = table  # (kept until the next call: the library copies it in stream order)
        _lib.check(
            self._lib.mythos_oxdna_debye_sweep(self._h, _lib.ptr(c), _lib.ptr(q), nf, nt, table.ctypes.data_as(_lib.c_double_p),
                                               _lib.ptr(e), _lib.ptr(de), _lib.stream(self.device)),
            "debye_sweep",
        )
        return e, de

    def order_params(self, center, quat, ops, *, raw=False, hb_cutoff=-0.1):
        """oxDNA's ``bond`` and ``mindistance`` order parameters of every frame (mythos_oxdna_order_params).  ``ops``: a
        sequence of ``mythos_amd.input.order_parameters.OrderParameter``.  Returns the (F, n_ops) float64 values - for
        ``bond`` the number of listed pairs whose hydrogen-bonding energy is below ``hb_cutoff``, for ``mindistance`` the
        smallest base-base distance of the listed pairs (the interfaces are applied by
        ``mythos_amd.observables.OrderParameters``) - and with ``raw`` also the (F, P) hydrogen-bonding energies and
        base-base distances of the listed pairs, all order parameters' lists one after the other.  oxDNA1, oxDNA2 and
        oxRNA2 systems with a discrete sequence; needs parameters, not neighbours."""
        from mythos_amd.input.order_parameters import KINDS

        c, q, nf, _ = self._frames(center, quat)
        cached = self._op_lists  # a trajectory is evaluated with one set of lists, call after call
        if cached is not None and (cached[0] is ops or cached[0] == ops):
            _, kind, first, pairs = cached
        else:
            ops = tuple(ops)
            kind = np.ascontiguousarray([KINDS.index(o.kind) for o in ops], dtype=np.int32)
            first = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(o.pairs) for o in ops])]), dtype=np.int32)
            pairs = np.ascontiguousarray([p for o in ops for p in o.pairs], dtype=np.int32).reshape(-1, 2)
            if pairs.size and int(pairs.max()) >= self.n:
                raise ValueError(f"an order parameter names nucleotide {int(pairs.max())}; the system has {self.n}")
            self._op_lists = (ops, kind, first, pairs)
        n_pairs = int(pairs.shape[0])
        out = torch.empty((nf, len(ops)), dtype=torch.float64, device=self.device)
        hb = torch.empty((nf, n_pairs), dtype=torch.float64, device=self.device) if raw else None
        dist = torch.empty((nf, n_pairs), dtype=torch.float64, device=self.device) if raw else None
        _lib.check(
            self._lib.mythos_oxdna_order_params(
                self._h, _lib.ptr(c), _lib.ptr(q), nf, len(ops), kind.ctypes.data_as(_lib.c_int_p), first.ctypes.data_as(_lib.c_int_p),
                pairs.ctypes.data_as(_lib.c_int_p), n_pairs, float(hb_cutoff), _lib.ptr(out), _lib.ptr(hb), _lib.ptr(dist),
                _lib.stream(self.device)),
            "order_params",
        )
        return (out, hb, dist) if raw else out


def _touched(*tensors) -> None:
    """The library has just written into these caller tensors through raw pointers: bump torch's version counters, so that
    anything keyed on them (the fused-observable rows of mythos_amd/observables/base.py) sees the change."""
    for t in tensors:
        if t is not None:
            torch.autograd.graph.increment_version(t)


class _MdIntegrator(_lib.Handle):
    """What the two Langevin integrators share: a handle of the C ABI whose entry points are named ``<_prefix>_*``
    (mythos_langevin_* / mythos_martini_langevin_*) - its creation on a system, the step counter and the figures of the
    last run.  The system is kept alive with it; closing the system first is allowed, using the integrator afterwards is not."""

    _prefix = ""
    _destroy = property(lambda self: f"{self._prefix}_destroy")

    def __init__(self, system, *args):
        self.system = system
        super().__init__(f"{self._prefix}_create", system._h, *args)

    def _fn(self, name):
        return getattr(self._lib, f"{self._prefix}_{name}")

    @property
    def step(self) -> int:
        return int(self._fn("get_step")(self._h))

    def set_timing(self, samples: int) -> None:
        """Bracket ``samples`` dispatches per run with HIP event pairs (0 = off, the default; see last_kernel_ms)."""
        _lib.check(self._fn("set_timing")(self._h, int(samples)), "set_timing")

    def _count(self, name: str) -> int:
        r = C.c_int(0)
        _lib.check(self._fn(name)(self._h, C.byref(r)), name)
        return int(r.value)

    def last_recoveries(self) -> int:
        """Out-of-turn list rebuilds of the last run (a particle left its skin early, or rows / buckets had to grow)."""
        return self._count("last_recoveries")

    def last_rebuilds(self) -> int:
        """Scheduled list rebuilds inside the last run / advance."""
        return self._count("last_rebuilds")

    def last_kernel_ms(self) -> dict:
        """HIP-event timings of the last run (see include/mythos_hip.h)."""
        k, loop, n, ns = C.c_double(0.0), C.c_double(0.0), C.c_int(0), C.c_int(0)
        _lib.check(self._fn("last_kernel_ms")(self._h, C.byref(k), C.byref(loop), C.byref(n), C.byref(ns)), "last_kernel_ms")
        return {"kernel_ms": k.value, "loop_ms_per_launch": loop.value, "launches": n.value, "samples": ns.value}


class LangevinIntegrator(_MdIntegrator):
    """BAOAB rigid-body Langevin dynamics bound to an :class:`OxdnaSystem`."""

    _prefix = "mythos_langevin"

    def __init__(self, system: OxdnaSystem, dt, kT, gamma_t, gamma_r, mass=1.0, inertia=(1.0, 1.0, 1.0), seed=0):
        inertia = np.ascontiguousarray(inertia, dtype=np.float64)
        super().__init__(system, float(dt), float(kT), float(gamma_t), float(gamma_r), float(mass),
                         inertia.ctypes.data_as(_lib.c_double_p), C.c_uint64(int(seed) & (2**64 - 1)))
        self.dt, self.kT = float(dt), float(kT)
        self.external_forces = (np.zeros(0, np.int32), np.zeros((0, 3), np.float64))
        self.restraints = None  # the set last handed to set_restraints (None: never called)
        self.point_forces = None  # the set last handed to set_point_forces (None: never called)

    def set_neighbor_policy(self, r_cut: float, skin: float, every: int) -> None:
        _lib.check(
            self._lib.mythos_langevin_set_neighbor_policy(self._h, float(r_cut), float(skin), int(every)),
            "set_neighbor_policy",
        )

    def set_unfused(self, on: bool = True) -> None:
        """oxNA systems: step through the two-launch path (forces launch + integrator launch) from the next load / run
        on - the second implementation the fused oxNA step kernel is checked against (mythos_langevin_set_option)."""
        _lib.check(self._lib.mythos_langevin_set_option(self._h, 0, 1 if on else 0), "set_option(unfused)")

    def set_external_forces(self, index=None, force=None) -> None:
        """Constant forces on the centres of mass of the listed nucleotides (oxDNA's ``string`` force with ``rate = 0``;
        mythos_langevin_set_external_forces): ``index`` (m,), ``force`` (m, 3); a nucleotide listed more than once gets the
        sum.  No arguments, or empty lists, clear them.  Refused between ``advance`` and ``store`` (an open frame).
        ``external_forces`` keeps what was handed to the library."""
        from mythos_amd.input.external_forces import sum_repeated

        if index is None or len(index) == 0:
            idx, f = np.zeros(0, np.int32), np.zeros((0, 3), np.float64)
        else:
            idx, f = sum_repeated(torch.as_tensor(index).detach().cpu().numpy(), torch.as_tensor(force).detach().cpu().numpy())
        idx, f = np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(f, dtype=np.float64)
        _lib.check(self._lib.mythos_langevin_set_external_forces(self._h, int(idx.shape[0]), idx.ctypes.data_as(_lib.c_int_p),
                                                                 f.ctypes.data_as(_lib.c_double_p)), "set_external_forces")
        self.external_forces = (idx, f)

    def set_restraints(self, restraints=None, reference_center=None, *, n_one=None, n_rep=1, offsets=None) -> None:
        """Position-dependent forces on centres of mass (mythos_amd.simulators.restraints; mythos_langevin_set_restraints):
        harmonic tethers, restraints of a sum of positions, torques on groups.  ``reference_center`` (n, 3): the state that
        ``anchor=None`` / ``target=None`` take their positions from.  None, or an empty set, clears them.  Refused between
        ``advance`` and ``store`` (an open frame).  ``restraints`` keeps the set; the keyword arguments repeat it per
        replica (Restraints.lower; HipMDSimulator passes them)."""
        from mythos_amd.simulators.restraints import Restraints

        rs = Restraints() if restraints is None else restraints
        if isinstance(reference_center, torch.Tensor):
            reference_center = reference_center.detach().double().cpu().numpy()
        a = rs.lower(reference_center, n_one=self.system.n if n_one is None else n_one, n_rep=n_rep, offsets=offsets)
        ip, dp = (lambda x: x.ctypes.data_as(_lib.c_int_p)), (lambda x: x.ctypes.data_as(_lib.c_double_p))
        _lib.check(self._lib.mythos_langevin_set_restraints(
            self._h, int(a["t_index"].shape[0]), ip(a["t_index"]), dp(a["t_k"]), dp(a["t_anchor"]), ip(a["t_mask"]),
            int(a["g_kind"].shape[0]), ip(a["g_kind"]), ip(a["g_first"]), ip(a["g_member"]), dp(a["g_vec"]), dp(a["g_target"]),
            ip(a["g_mask"])), "set_restraints")
        self.restraints = rs

    def external_field(self, center):
        """The external field at ``center`` (n, 3) - constant forces, tethers, sum restraints, torques - evaluated by the
        kernels the integrator kicks with (mythos_langevin_eval_external): -> (force (n, 3) in the system's precision,
        energies (3,) float64: -sum F.x of the constant forces, the tether energy, the sum-restraint energy; the torque
        has no potential).  Needs no resident state and changes none."""
        s = self.system
        c = s._check(center, (s.n, 3), "center")
        force = torch.empty((s.n, 3), dtype=s.dtype, device=s.device)
        energies = torch.empty(3, dtype=torch.float64, device=s.device)
        _lib.check(self._lib.mythos_langevin_eval_external(self._h, _lib.ptr(c), _lib.ptr(force), _lib.ptr(energies), _lib.stream(s.device)),
                   "eval_external")
        return force, energies

    def set_point_forces(self, point_forces=None, *, n_one=None, n_rep=1, offsets=None) -> None:
        """oxDNA's point forces on single nucleotides (mythos_amd.simulators.restraints.PointForces: moving strings, traps,
        mutual traps, repulsion planes and spheres; mythos_langevin_set_point_forces).  The moving ones take the
        integrator's step count (``step``) as their time.  A set of its own beside ``set_restraints`` and
        ``set_external_forces``: all three add up.  None, or an empty set, clears it.  Refused between ``advance`` and
        ``store`` (an open frame).  The keyword arguments repeat the set per replica (PointForces.lower)."""
        from mythos_amd.simulators.restraints import PointForces

        pf = PointForces() if point_forces is None else point_forces
        a = pf.lower(n_one=self.system.n if n_one is None else n_one, n_rep=n_rep, offsets=offsets)
        ip = lambda x: x.ctypes.data_as(_lib.c_int_p)  # noqa: E731
        _lib.check(self._lib.mythos_langevin_set_point_forces(
            self._h, int(a["kind"].shape[0]), ip(a["kind"]), ip(a["particle"]), ip(a["ref_particle"]), ip(a["flags"]),
            a["param"].ctypes.data_as(_lib.c_double_p)), "set_point_forces")
        self.point_forces = pf

    def external_field_at(self, center, step):
        """``external_field`` at step count ``step``, with the point forces: -> (force (n, 3), energies (8,) float64: the
        three of ``external_field``, then the energy of the point terms of each kind - string, trap, mutual trap,
        repulsion plane, repulsion sphere (mythos_langevin_eval_external_at)."""
        s = self.system
        c = s._check(center, (s.n, 3), "center")
        force = torch.empty((s.n, 3), dtype=s.dtype, device=s.device)
        energies = torch.empty(8, dtype=torch.float64, device=s.device)
        _lib.check(self._lib.mythos_langevin_eval_external_at(self._h, _lib.ptr(c), float(step), _lib.ptr(force), _lib.ptr(energies),
                                                              _lib.stream(s.device)), "eval_external_at")
        return force, energies

    def init_momenta(self):
        s = self.system
        p = torch.empty((s.n, 3), dtype=s.dtype, device=s.device)
        ang = torch.empty((s.n, 3), dtype=s.dtype, device=s.device)
        _lib.check(self._lib.mythos_langevin_init_momenta(self._h, _lib.ptr(p), _lib.ptr(ang), _lib.stream(s.device)), "init_momenta")
        return p, ang

    def run(self, center, quat, p_lin, p_ang, n_steps: int, save_every: int = 0, want_energy: bool = True):
        """Advance in place; returns (traj_center, traj_quat, e_trace) or Nones when save_every == 0."""
        state = self._state_ptrs(center, quat, p_lin, p_ang)
        tc, tq, et = self._rows(n_steps, save_every, want_energy)
        rc = self._lib.mythos_langevin_run(
            self._h, *state, int(n_steps), int(save_every), _lib.ptr(tc), _lib.ptr(tq), _lib.ptr(et), _lib.stream(self.system.device),
        )
        _touched(center, quat, p_lin, p_ang)  # (a run that fails still hands back the state of its last valid step)
        _lib.check(rc, "langevin_run")
        return tc, tq, et

    def _state_ptrs(self, center, quat, p_lin, p_ang):
        s = self.system
        for t, tail, name in ((center, (s.n, 3), "center"), (quat, (s.n, 4), "quat"), (p_lin, (s.n, 3), "p_lin"), (p_ang, (s.n, 3), "p_ang")):
            if s._check(t, tail, name).data_ptr() != t.data_ptr():
                raise ValueError(f"{name} must be contiguous (the library reads and writes it in place)")
        return _lib.ptr(center), _lib.ptr(quat), _lib.ptr(p_lin), _lib.ptr(p_ang)

    def _rows(self, n_steps: int, save_every: int, want_energy: bool, out=None):
        """Rows for the saved steps: (traj_center, traj_quat, e_trace), Nones where there is nothing to save.
        ``out = (traj_center, traj_quat)``: the caller's tensors, checked, instead of new ones."""
        s = self.system
        n_save = n_steps // save_every if save_every > 0 else 0
        if out is not None and n_save:
            tc, tq = out
            for t, w in ((tc, 3), (tq, 4)):
                if t.device != s.device or t.dtype != s.dtype or tuple(t.shape) != (n_save, s.n, w) or not t.is_contiguous():
                    raise ValueError(f"out tensors must be contiguous {s.dtype} of shape ({n_save}, {s.n}, 3) and ({n_save}, {s.n}, 4) on {s.device}")
        else:
            tc = torch.empty((n_save, s.n, 3), dtype=s.dtype, device=s.device) if n_save else None
            tq = torch.empty((n_save, s.n, 4), dtype=s.dtype, device=s.device) if n_save else None
        et = torch.zeros((n_save, TRACE_WIDTH), dtype=torch.float64, device=s.device) if (n_save and want_energy) else None
        return tc, tq, et

    # ---- resident form: the state stays in the integrator's layout on the device between calls ----------
    def load(self, center, quat, p_lin, p_ang) -> None:
        """Copy a state into the integrator (mythos_langevin_load); ``advance`` then steps it in place."""
        _lib.check(self._lib.mythos_langevin_load(self._h, *self._state_ptrs(center, quat, p_lin, p_ang), _lib.stream(self.system.device)), "langevin_load")

    def advance(self, n_steps: int, save_every: int = 0, want_energy: bool = True, out=None):
        """``n_steps`` on the resident state; the neighbour list and its rebuild schedule carry over between calls.
        Returns (traj_center, traj_quat, e_trace) or Nones when save_every == 0.  ``out = (traj_center, traj_quat)``:
        rows written into the caller's tensors ((n_steps // save_every, n, 3 | 4), contiguous) instead of new ones."""
        s = self.system
        tc, tq, et = self._rows(n_steps, save_every, want_energy, out)
        _lib.check(
            self._lib.mythos_langevin_advance(self._h, int(n_steps), int(save_every), _lib.ptr(tc), _lib.ptr(tq), _lib.ptr(et), _lib.stream(s.device)),
            "langevin_advance",
        )
        if out is not None and tc is not None:
            _touched(tc, tq)
        return tc, tq, et

    def store(self, center, quat, p_lin, p_ang) -> None:
        """Copy the resident state out (mythos_langevin_store, asynchronous on the current stream)."""
        rc = self._lib.mythos_langevin_store(self._h, *self._state_ptrs(center, quat, p_lin, p_ang), _lib.stream(self.system.device))
        _touched(center, quat, p_lin, p_ang)  # (the arrays are written even when closing an open frame failed)
        _lib.check(rc, "langevin_store")

    # ---- umbrella sampling on the resident state (mythos_amd.simulators.umbrella) -----------------------
    def set_umbrella(self, ops=None, table=None, segment_steps: int = 50, n_rep: int = 1, hb_cutoff: float = -0.1) -> None:
        """Bias the resident dynamics by a weights table over the states of ``ops`` (``bond`` / ``mindistance``
        ``OrderParameter``s or the path of their file, naming nucleotides of ONE of the ``n_rep`` replicas;
        mythos_langevin_set_umbrella).  ``table``: {state tuple: weight} or an array with one axis per order parameter
        (``lower_table``).  ``segment_steps``: steps per proposal.  No arguments clear the bias.  Refused between ``advance``
        and ``store`` (an open frame), for moving point forces, oxNA systems and a probabilistic sequence."""
        from mythos_amd.simulators import umbrella as U

        if ops is None:
            _lib.check(self._lib.mythos_langevin_set_umbrella(self._h, 1, 0, None, None, None, 0, None, None, None, None, float(hb_cutoff), 1),
                       "set_umbrella")
            self._umbrella_ops = ()
            return
        ops = U.as_order_parameters(ops)
        dense = U.lower_table(ops, table)
        keep, args = U._bias_args(ops, dense)
        _lib.check(self._lib.mythos_langevin_set_umbrella(self._h, int(n_rep), *args, float(hb_cutoff), int(segment_steps)), "set_umbrella")
        del keep
        self._umbrella_ops, self._umbrella_rep = ops, int(n_rep)

    def advance_umbrella(self, n_segments: int, sample_every: int = 1, proposals: bool = False):
        """``n_segments`` segments of the biased chain on the resident state (mythos_langevin_advance_umbrella) ->
        (traj_center (S, n, 3), traj_quat (S, n, 4), ``UmbrellaRecord``), S = n_segments // sample_every rows holding the
        state after the decision of every ``sample_every``-th boundary (``sample_every = 0``: no rows, Nones).  The record's
        tensors have the leading shape (n_segments, n_rep); ``proposals``: it also carries the proposals' rows."""
        from mythos_amd.simulators import umbrella as U

        ops = getattr(self, "_umbrella_ops", ())
        if not ops:
            raise ValueError("advance_umbrella: no bias is set (set_umbrella)")
        s = self.system
        n_seg, n_rep = int(n_segments), self._umbrella_rep
        n_save = n_seg // sample_every if sample_every > 0 else 0
        rows = lambda w: torch.empty((n_save, s.n, w), dtype=s.dtype, device=s.device) if n_save else None  # noqa: E731
        tc, tq = rows(3), rows(4)
        pc, pq = (rows(3), rows(4)) if proposals else (None, None)
        raw = torch.zeros((n_seg, n_rep, 3 * len(ops) + 4), dtype=torch.float64, device=s.device)
        _lib.check(self._lib.mythos_langevin_advance_umbrella(self._h, n_seg, int(sample_every), _lib.ptr(tc), _lib.ptr(tq), _lib.ptr(pc),
                                                              _lib.ptr(pq), _lib.ptr(raw), _lib.stream(s.device)), "advance_umbrella")
        return tc, tq, U.record_of(raw, len(ops), pc, pq)

    def umbrella_counts(self) -> tuple[int, int]:
        """(accepted, decided) decisions since ``set_umbrella`` (mythos_langevin_umbrella_counts)."""
        a, d = C.c_int64(0), C.c_int64(0)
        _lib.check(self._lib.mythos_langevin_umbrella_counts(self._h, C.byref(a), C.byref(d)), "umbrella_counts")
        return int(a.value), int(d.value)

    @_MdIntegrator.step.setter
    def step(self, value: int) -> None:
        _lib.check(self._lib.mythos_langevin_set_step(self._h, int(value)), "set_step")

    def set_seed(self, seed: int) -> None:
        """Key of the noise from the next launch / init_momenta on (mythos_langevin_set_seed)."""
        _lib.check(self._lib.mythos_langevin_set_seed(self._h, C.c_uint64(int(seed) & (2**64 - 1))), "set_seed")


def martini_frames(pos, box):
    """pos (F, N, 3) or (N, 3), box (F, 3), (1, 3) or (3,) -> contiguous (F, N, 3) and (F, 3) of pos's dtype on its device:
    what every MARTINI entry point of the library reads (a box row per frame).  For the energy calls and the observables."""
    if box is None:
        raise ValueError("MARTINI observables need trajectory.box_size (per-frame periodic box)")
    if not isinstance(pos, torch.Tensor) or pos.device.type != "cuda":
        raise _lib.MythosHipError("observables are evaluated by the HIP library: the trajectory must live on a GPU "
                                  "(mythos_amd has no CPU fallback)")
    if pos.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"unsupported dtype {pos.dtype}")
    if pos.dim() == 2:
        pos = pos[None]
    box = torch.as_tensor(box, dtype=pos.dtype, device=pos.device).reshape(-1, 3)
    if box.shape[0] == 1 and pos.shape[0] > 1:
        box = box.expand(pos.shape[0], 3)
    if box.shape[0] != pos.shape[0]:
        raise ValueError(f"box_size has {box.shape[0]} rows for {pos.shape[0]} frames")
    return pos.contiguous(), box.contiguous()


class MartiniSystem(_lib.Handle):
    """One MARTINI system on one GPU (mythos_martini_t): LJ type tables, bonds, angles."""

    N_TERMS = 3  # lj, bond, angle
    _destroy = "mythos_martini_destroy"

    def __init__(self, types, sigma, eps, bonds, bond_k, bond_r0, angles, angle_k, angle_t0, angle_kind=0, r_cut=1.1,
                 dtype=torch.float32, device=None):
        if _lib.device_count() == 0 or not torch.cuda.is_available():
            raise _lib.MythosHipError("no HIP device visible: the mythos_amd HIP path has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.dtype = dtype
        types = np.ascontiguousarray(types, dtype=np.int32)
        self.n = int(types.shape[0])
        sigma = np.ascontiguousarray(sigma, dtype=np.float64)
        eps = np.ascontiguousarray(eps, dtype=np.float64)
        n_types = int(sigma.shape[0])
        bonds = np.ascontiguousarray(bonds, dtype=np.int32).reshape(-1, 2)
        angles = np.ascontiguousarray(angles, dtype=np.int32).reshape(-1, 3)
        self.n_types, self.n_bonds, self.n_angles = n_types, int(bonds.shape[0]), int(angles.shape[0])
        self.r_cut = float(r_cut)
        f = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
        bond_k, bond_r0, angle_k, angle_t0 = f(bond_k), f(bond_r0), f(angle_k), f(angle_t0)
        dp = lambda a: a.ctypes.data_as(_lib.c_double_p)  # noqa: E731
        super().__init__(
            "mythos_martini_create", self.n, types.ctypes.data_as(_lib.c_int_p), n_types, dp(sigma), dp(eps), int(bonds.shape[0]),
            bonds.ctypes.data_as(_lib.c_int_p), dp(bond_k), dp(bond_r0), int(angles.shape[0]),
            angles.ctypes.data_as(_lib.c_int_p), dp(angle_k), dp(angle_t0), int(angle_kind), float(r_cut),
            _lib.dtype_code(dtype), self.device.index or 0,
        )
        self.charged = False

    def set_charges(self, charges=None, epsilon_r: float = 15.0, epsilon_rf: float = 0.0) -> None:
        """Bead charges (e) for reaction-field Coulomb with the system's cut-off (mythos_martini_set_charges): relative
        permittivity ``epsilon_r`` inside it, ``epsilon_rf`` beyond (0: infinity) - GROMACS' ``epsilon_r`` / ``epsilon_rf``.
        ``None`` or all zeros clears them: the system then behaves as one that never had any.  An integrator of this
        system takes the charges with its next call."""
        q = None
        if charges is not None:
            q = np.ascontiguousarray(charges, dtype=np.float64)
            if q.shape != (self.n,):
                raise ValueError(f"charges must have shape ({self.n},)")
        _lib.check(self._lib.mythos_martini_set_charges(self._h, None if q is None else q.ctypes.data_as(_lib.c_double_p),
                                                        float(epsilon_r), float(epsilon_rf)), "martini_set_charges")
        self.charged = q is not None and bool(np.any(q != 0.0))

    def set_params(self, sigma=None, eps=None, bond_k=None, bond_r0=None, angle_k=None, angle_t0=None) -> None:
        """New values for the parameter tables, in place (mythos_martini_set_params; shapes as at creation, ``None`` keeps a
        table): the handle stays, and so does every integrator bound to it, which takes the tables with its next call."""
        shapes = ((self.n_types, self.n_types), (self.n_types, self.n_types), (self.n_bonds,), (self.n_bonds,), (self.n_angles,),
                  (self.n_angles,))
        arrs = []
        for a, shape, name in zip((sigma, eps, bond_k, bond_r0, angle_k, angle_t0), shapes, ("sigma", "eps", "bond_k", "bond_r0", "angle_k", "angle_t0")):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.shape != shape:
                    raise ValueError(f"{name} must have shape {shape}")
            arrs.append(a)
        _lib.check(self._lib.mythos_martini_set_params(self._h, *(None if a is None else a.ctypes.data_as(_lib.c_double_p) for a in arrs)),
                   "martini_set_params")

    def coulomb(self, pos: torch.Tensor, box: torch.Tensor, grads: bool = False):
        """pos (F, N, 3) or (N, 3); box (F, 3) or (3,) -> (reaction-field Coulomb energy (F,) float64 - pairs, excluded
        pairs and the self term -, dU/dpos or None).  Zero for a system without charges."""
        single = pos.dim() == 2
        pos, box = self._frames(pos, box)
        nf = pos.shape[0]
        e = torch.empty((nf,), dtype=torch.float64, device=self.device)
        g = torch.empty_like(pos) if grads else None
        _lib.check(
            self._lib.mythos_martini_coulomb(self._h, _lib.ptr(pos), _lib.ptr(box), nf, _lib.ptr(e), _lib.ptr(g), _lib.stream(self.device)),
            "martini_coulomb",
        )
        return (e[0], g[0] if grads else None) if single else (e, g)

    def _frames(self, pos, box):
        """``martini_frames`` of positions that are this system's: its dtype, device and number of beads."""
        if pos.device != self.device or pos.dtype != self.dtype or tuple(pos.shape[-2:]) != (self.n, 3):
            raise ValueError(f"pos must be a {self.dtype} tensor of shape (F, {self.n}, 3) on {self.device}")
        return martini_frames(pos, box)

    def energy(self, pos: torch.Tensor, box: torch.Tensor, grads: bool = False):
        """pos (F, N, 3) or (N, 3); box (F, 3) or (3,) -> (e_terms (F, 3) float64, dU/dpos or None)."""
        single = pos.dim() == 2
        pos, box = self._frames(pos, box)
        nf = pos.shape[0]
        e = torch.empty((nf, 3), dtype=torch.float64, device=self.device)
        g = torch.empty_like(pos) if grads else None
        _lib.check(
            self._lib.mythos_martini_energy(self._h, _lib.ptr(pos), _lib.ptr(box), nf, _lib.ptr(e), _lib.ptr(g), _lib.stream(self.device)),
            "martini_energy",
        )
        return (e[0], g[0] if grads else None) if single else (e, g)

    @staticmethod
    def check_stress_profile(n: int, r_cut: float, boxes, n_bins: int, center_index=None) -> None:
        """The host-side refusals of ``stress_profile`` alone (mythos_martini_stress_profile_check; no GPU): ``n_bins``
        outside [1, 1024], a centre index outside [0, n), a box edge (``boxes`` (F, 3) on the host, or None) that is not
        positive and finite or is below 2 ``r_cut`` - ``ValueError`` naming the offender."""
        b = None if boxes is None else np.ascontiguousarray(np.asarray(boxes, dtype=np.float64).reshape(-1, 3))
        c = np.ascontiguousarray([] if center_index is None else center_index, dtype=np.int32).reshape(-1)
        _lib.check(_lib.load().mythos_martini_stress_profile_check(
            int(n), float(r_cut), 0 if b is None else int(b.shape[0]), None if b is None else b.ctypes.data_as(_lib.c_double_p),
            int(c.size), c.ctypes.data_as(_lib.c_int_p), int(n_bins)), "martini_stress_profile_check")

    def stress_profile(self, pos: torch.Tensor, box: torch.Tensor, n_bins: int, center_index=None, by_term: bool = False,
                       check_boxes: bool = True) -> torch.Tensor:
        """Raw rows of the lateral pressure profile (mythos_martini_stress_profile): pos (F, N, 3) or
        (N, 3), box (F, 3) or (3,) -> (F, n_bins, 4) float64 on the device - bead count, W_x, W_y, W_z (kJ/mol) of every
        slab along z - or with ``by_term`` (F, n_bins, 13): the count, then W of lj, bond, angle, coulomb.
        ``center_index``: beads whose mean stored z is the frame's midplane (slab n_bins / 2 starts there); None: slabs
        fixed to the box.  Reading the boxes for the edge checks is one host synchronisation per call;
        ``check_boxes=False`` leaves them on the device - for boxes already validated (``check_stress_profile``) - and the call
        then queues its launches without synchronising, as the C entry point does."""
        pos, box = self._frames(pos, box)
        nf = pos.shape[0]
        c = np.ascontiguousarray([] if center_index is None else center_index, dtype=np.int32).reshape(-1)
        self.check_stress_profile(self.n, self.r_cut, box.detach().to("cpu", torch.float64).numpy() if check_boxes else None, n_bins, c)
        out = torch.empty((nf, int(n_bins), _lib.STRESS_ROW_BY_TERM if by_term else _lib.STRESS_ROW), dtype=torch.float64, device=self.device)
        _lib.check(self._lib.mythos_martini_stress_profile(self._h, _lib.ptr(pos), _lib.ptr(box), nf, int(c.size), c.ctypes.data_as(_lib.c_int_p),
                                                           int(n_bins), 1 if by_term else 0, _lib.ptr(out), _lib.stream(self.device)),
                   "martini_stress_profile")
        return out

    def param_grads(self, pos: torch.Tensor, box: torch.Tensor, lj: bool = True, bonds: bool = True, angles: bool = True):
        """Per-frame parameter gradients (float64, on the device): dict with ``sigma``/``eps`` (F, T, T) for the
        ordered type pair, ``bond_k``/``bond_r0`` (F, n_bonds), ``angle_k``/``angle_t0`` (F, n_angles)."""
        pos, box = self._frames(pos, box)
        nf = pos.shape[0]

        def buf(on, *shape):
            return torch.zeros((nf, *shape), dtype=torch.float64, device=self.device) if on else None

        out = {"sigma": buf(lj, self.n_types, self.n_types), "eps": buf(lj, self.n_types, self.n_types),
               "bond_k": buf(bonds, self.n_bonds), "bond_r0": buf(bonds, self.n_bonds),
               "angle_k": buf(angles, self.n_angles), "angle_t0": buf(angles, self.n_angles)}
        _lib.check(
            self._lib.mythos_martini_param_grads(
                self._h, _lib.ptr(pos), _lib.ptr(box), nf, _lib.ptr(out["sigma"]), _lib.ptr(out["eps"]),
                _lib.ptr(out["bond_k"]), _lib.ptr(out["bond_r0"]), _lib.ptr(out["angle_k"]), _lib.ptr(out["angle_t0"]),
                _lib.stream(self.device)),
            "martini_param_grads",
        )
        return out


class MartiniLangevinIntegrator(_MdIntegrator):
    """BAOAB Langevin dynamics of a :class:`MartiniSystem` (mythos_martini_sim_t): LJ over a device-built Verlet
    list, bonds, angles, and reaction-field Coulomb when the system holds charges; units nm, ps, amu, kJ/mol.
    ``gamma`` is the friction rate in 1/ps."""

    KB = 0.0083144626  # kJ/mol/K
    _prefix = "mythos_martini_langevin"

    def __init__(self, system: MartiniSystem, dt, kT, gamma, mass=None, seed=0):
        mptr = None
        if mass is not None:
            mass = np.ascontiguousarray(mass, dtype=np.float64)
            if mass.shape != (system.n,):
                raise ValueError(f"mass must have shape ({system.n},)")
            mptr = mass.ctypes.data_as(_lib.c_double_p)
        super().__init__(system, float(dt), float(kT), float(gamma), mptr, int(seed))

    def set_neighbor_policy(self, skin: float, every: int) -> None:
        _lib.check(self._lib.mythos_martini_langevin_set_neighbor_policy(self._h, float(skin), int(every)), "set_neighbor_policy")

    def set_inner_list(self, margin: float, every: int) -> None:
        """Pruned rows inside r_cut + ``margin``, rewritten every ``every`` steps by the step launch (off by default;
        margin <= 0 switches them off again) - include/mythos_hip.h."""
        _lib.check(self._lib.mythos_martini_langevin_set_inner_list(self._h, float(margin), int(every)), "set_inner_list")

    BAROSTATS = {None: 0, "berendsen": 1, "c-rescale": 2}  # the reference's mdp key ``pcoupl``
    COUPLINGS = {"isotropic": 0, "semiisotropic": 1}         # ``pcoupltype``

    def set_barostat(self, kind=None, coupling="isotropic", ref_p=1.0, compressibility=4.5e-5, tau_p=1.0, every=10) -> None:
        """Pressure coupling by cell rescaling (mythos_martini_langevin_set_barostat): ``kind`` None (off), "berendsen" or
        "c-rescale" (stochastic cell rescaling); ``coupling`` "isotropic" or "semiisotropic", for which ``ref_p`` (bar) and
        ``compressibility`` (1/bar) are (xy, z) pairs - a scalar serves both; ``tau_p`` in ps; an event every ``every``
        steps of the integrator's step counter.  GROMACS' ``ref-p``, ``compressibility``, ``tau-p``, ``nstpcouple``."""
        if kind not in self.BAROSTATS or coupling not in self.COUPLINGS:
            raise ValueError(f"kind must be one of {list(self.BAROSTATS)}, coupling one of {list(self.COUPLINGS)}")
        pair = lambda v: np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (2,)))  # noqa: E731
        p0, beta = pair(ref_p), pair(compressibility)
        _lib.check(self._lib.mythos_martini_langevin_set_barostat(
            self._h, self.BAROSTATS[kind], self.COUPLINGS[coupling], p0.ctypes.data_as(_lib.c_double_p),
            beta.ctypes.data_as(_lib.c_double_p), float(tau_p), int(every)), "set_barostat")

    def pressure(self) -> dict:
        """Pressure of the resident state (mythos_martini_langevin_pressure; synchronises): ``kinetic`` and ``virial``
        (3,) float64 in kJ/mol - sum m v_d^2 and -dU/dln s_d -, ``pressure`` (3,) in bar, ``volume`` in nm^3 and the
        scalar ``p`` = mean of the three.  An open frame is closed first, as ``store`` does."""
        out = np.zeros(10, dtype=np.float64)
        _lib.check(self._lib.mythos_martini_langevin_pressure(self._h, out.ctypes.data_as(_lib.c_double_p), _lib.stream(self.system.device)),
                   "martini_langevin_pressure")
        return {"kinetic": out[0:3].copy(), "virial": out[3:6].copy(), "pressure": out[6:9].copy(), "volume": float(out[9]),
                "p": float(out[6:9].mean())}

    @property
    def box(self) -> np.ndarray:
        """(3,) float64: the box of the resident state - the one loaded, rescaled by the coupling events since."""
        b = np.zeros(3, dtype=np.float64)
        _lib.check(self._lib.mythos_martini_langevin_get_box(self._h, b.ctypes.data_as(_lib.c_double_p)), "get_box")
        return b

    @property
    def last_boxes(self) -> torch.Tensor:
        """(S, 3) float64 on the system's device: the box of every row the last ``run`` / ``advance`` saved - what
        ``SimulatorTrajectory.box_size`` takes.  A row saved at a coupling step is the state before the event, with its box."""
        n = C.c_int(0)
        _lib.check(self._lib.mythos_martini_langevin_last_boxes(self._h, None, C.byref(n)), "last_boxes")
        b = np.zeros((n.value, 3), dtype=np.float64)
        if n.value:
            _lib.check(self._lib.mythos_martini_langevin_last_boxes(self._h, b.ctypes.data_as(_lib.c_double_p), C.byref(n)), "last_boxes")
        return torch.as_tensor(b, device=self.system.device)

    def init_velocities(self) -> torch.Tensor:
        v = torch.empty((self.system.n, 3), dtype=self.system.dtype, device=self.system.device)
        _lib.check(self._lib.mythos_martini_langevin_init_velocities(self._h, _lib.ptr(v), _lib.stream(self.system.device)), "init_velocities")
        return v

    def _check_state(self, pos, vel):
        s = self.system
        for t, name in ((pos, "pos"), (vel, "vel")):
            if t.device != s.device or t.dtype != s.dtype or tuple(t.shape) != (s.n, 3) or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous {s.dtype} tensor of shape ({s.n}, 3) on {s.device}")

    def _rows(self, n_steps: int, save_every: int, want_energy: bool):
        s = self.system
        ns = n_steps // save_every if save_every > 0 else 0
        traj = torch.empty((ns, s.n, 3), dtype=s.dtype, device=s.device) if ns else None
        # (a fifth column, the Coulomb energy, when the system holds charges: include/mythos_hip.h)
        et = torch.zeros((ns, 5 if s.charged else 4), dtype=torch.float64, device=s.device) if (ns and want_energy) else None
        return traj, et

    def run(self, pos, vel, box, n_steps: int, save_every: int = 0, want_energy: bool = True):
        """Advance ``pos`` / ``vel`` (n, 3) in place -> (traj_pos (S, n, 3) or None, e_trace (S, 4) float64 or None);
        e_trace columns: lj, bond, angle, kinetic (kJ/mol) at the saved steps (``want_energy=False``: positions only), and
        a fifth, the reaction-field Coulomb energy, when the system holds charges (``MartiniSystem.set_charges``)."""
        s = self.system
        self._check_state(pos, vel)
        box = np.ascontiguousarray(np.asarray(box, dtype=np.float64).reshape(3))
        traj, et = self._rows(n_steps, save_every, want_energy)
        rc = self._lib.mythos_martini_langevin_run(
            self._h, _lib.ptr(pos), _lib.ptr(vel), box.ctypes.data_as(_lib.c_double_p), int(n_steps), int(save_every),
            _lib.ptr(traj), _lib.ptr(et), _lib.stream(s.device))
        _touched(pos, vel)
        _lib.check(rc, "martini_langevin_run")
        return traj, et

    # ---- resident form (mythos_martini_langevin_load / advance / store) -----------------------------------
    def load(self, pos, vel, box) -> None:
        self._check_state(pos, vel)
        box = np.ascontiguousarray(np.asarray(box, dtype=np.float64).reshape(3))
        _lib.check(self._lib.mythos_martini_langevin_load(self._h, _lib.ptr(pos), _lib.ptr(vel), box.ctypes.data_as(_lib.c_double_p),
                                                          _lib.stream(self.system.device)), "martini_langevin_load")

    def advance(self, n_steps: int, save_every: int = 0, want_energy: bool = True):
        """``n_steps`` on the resident state: n launches, the frame stays open; the list and its schedule carry over."""
        traj, et = self._rows(n_steps, save_every, want_energy)
        _lib.check(self._lib.mythos_martini_langevin_advance(self._h, int(n_steps), int(save_every), _lib.ptr(traj), _lib.ptr(et),
                                                             _lib.stream(self.system.device)), "martini_langevin_advance")
        return traj, et

    def store(self, pos, vel) -> None:
        self._check_state(pos, vel)
        rc = self._lib.mythos_martini_langevin_store(self._h, _lib.ptr(pos), _lib.ptr(vel), _lib.stream(self.system.device))
        _touched(pos, vel)
        _lib.check(rc, "martini_langevin_store")

    def rows(self, pruned: bool = False):
        """(rows (n, stride) int32, lengths (n,) int32) of the Verlet rows, or of the pruned rows, as numpy arrays
        (diagnostics / tests; synchronises)."""
        stride = C.c_int(0)
        which = 1 if pruned else 0
        _lib.check(self._lib.mythos_martini_langevin_get_rows(self._h, which, None, None, C.byref(stride)), "get_rows")
        rows = np.empty((self.system.n, stride.value), dtype=np.int32)
        lens = np.empty(self.system.n, dtype=np.int32)
        _lib.check(self._lib.mythos_martini_langevin_get_rows(self._h, which, rows.ctypes.data_as(C.POINTER(C.c_int32)),
                                                              lens.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(stride)), "get_rows")
        return rows, lens

    def neighbor_stats(self) -> tuple[int, float]:
        mx, mean = C.c_int(0), C.c_double(0.0)
        _lib.check(self._lib.mythos_martini_langevin_neighbor_stats(self._h, C.byref(mx), C.byref(mean)), "neighbor_stats")
        return mx.value, mean.value

    # ---- position restraints, flat-bottomed restraints, pulling (mythos_amd.simulators.martini_restraints) ---------
    _replicas = 1      # leading replica axis of the tensors below: none for the single integrator
    restraints = None  # the set last handed to set_restraints

    def _lead(self) -> tuple:
        return ()

    def set_restraints(self, restraints=None, reference_pos=None, *, box=None, topology=None) -> None:
        """External forces on the beads (mythos_martini_langevin_set_restraints): a ``MartiniRestraints`` set of position
        restraints, flat-bottomed restraints and pull coordinates between centres of mass.  ``reference_pos``: the state
        that references left ``None`` take their positions from; ``box``: the box(es) of the state, for periodic
        coordinates and ``pbc_ref`` (default: those of the resident state); ``topology``: for groups given by a selection.
        None, or an empty set, clears them: the integrator then launches what it launched before.  Refused together with
        a barostat or replica exchange, and between ``advance`` and ``store`` (an open frame)."""
        from mythos_amd.simulators import martini_restraints as mr

        rs = mr.MartiniRestraints() if restraints is None else restraints
        if isinstance(reference_pos, torch.Tensor):
            reference_pos = reference_pos.detach().double().cpu().numpy()
        if box is None and rs:
            b = self.box
            box = b if np.all(b > 0) else None
        a = rs.lower(topology, n_rep=self._replicas, boxes=box, reference_pos=reference_pos)
        _lib.check(self._lib.mythos_martini_langevin_set_restraints(self._h, *mr.c_args(a)), "martini_set_restraints")
        self.restraints = rs

    def _n_pull(self) -> int:
        return int(self._lib.mythos_martini_langevin_n_pull(self._h))

    def external_field(self, pos, step=None):
        """The external field at ``pos`` and step count ``step`` (default: the integrator's), evaluated by the kernels the
        integrator kicks with (mythos_martini_langevin_eval_external): -> (force like ``pos``, energies (4,) float64 -
        position, flat-bottom, umbrella, constant-force -, xi (P,) float64: the pull coordinates).  The ensemble's carry
        its leading replica axis.  Needs no resident state and changes none."""
        s = self.system
        shape = (*self._lead(), s.n, 3)
        if pos.device != s.device or pos.dtype != s.dtype or tuple(pos.shape) != shape or not pos.is_contiguous():
            raise ValueError(f"pos must be a contiguous {s.dtype} tensor of shape {shape} on {s.device}")
        force = torch.empty_like(pos)
        energies = torch.zeros((*self._lead(), 4), dtype=torch.float64, device=s.device)
        xi = torch.zeros((*self._lead(), self._n_pull()), dtype=torch.float64, device=s.device)
        _lib.check(self._lib.mythos_martini_langevin_eval_external(self._h, _lib.ptr(pos), float(self.step if step is None else step),
                                                                   _lib.ptr(force), _lib.ptr(energies), _lib.ptr(xi), _lib.stream(s.device)),
                   "martini_eval_external")
        return force, energies, xi

    def pull_values(self, pos) -> torch.Tensor:
        """xi of every pull coordinate on a stored trajectory ``pos`` (rows, n, 3) - the ensemble's (rows, R, n, 3) -
        -> (rows, P) / (rows, R, P) float64 on the device (mythos_martini_langevin_pull_values)."""
        s = self.system
        tail = (*self._lead(), s.n, 3)
        if pos.device != s.device or pos.dtype != s.dtype or pos.dim() != len(tail) + 1 or tuple(pos.shape[1:]) != tail:
            raise ValueError(f"pos must be a {s.dtype} tensor of shape (rows, {', '.join(map(str, tail))}) on {s.device}")
        pos = pos.contiguous()
        out = torch.zeros((pos.shape[0], *self._lead(), self._n_pull()), dtype=torch.float64, device=s.device)
        _lib.check(self._lib.mythos_martini_langevin_pull_values(self._h, _lib.ptr(pos), int(pos.shape[0]), _lib.ptr(out),
                                                                 _lib.stream(s.device)), "martini_pull_values")
        return out


class _MartiniEnsembleHandle(MartiniLangevinIntegrator):
    """The handle behind :class:`MartiniEnsembleIntegrator` (mythos_martini_langevin_create_ensemble): the single
    integrator's entry points on tensors with a leading replica axis."""

    def __init__(self, system: MartiniSystem, dt, kT, gamma, mass=None, seeds=None):
        kT = np.ascontiguousarray(np.atleast_1d(np.asarray(kT, dtype=np.float64)))
        if kT.ndim != 1 or kT.size < 1:
            raise ValueError("kT must be a non-empty sequence, one value per replica")
        self.n_rep = int(kT.size)
        if seeds is None or np.isscalar(seeds):
            seeds = [(int(seeds or 0) + r) & (2**64 - 1) for r in range(self.n_rep)]
        seeds = np.ascontiguousarray(np.asarray([int(s) & (2**64 - 1) for s in seeds], dtype=np.uint64))
        if seeds.shape != (self.n_rep,):
            raise ValueError(f"seeds must be an int or {self.n_rep} values, one per replica")
        mptr = None
        if mass is not None:
            mass = np.ascontiguousarray(mass, dtype=np.float64)
            if mass.shape != (system.n,):
                raise ValueError(f"mass must have shape ({system.n},)")
            mptr = mass.ctypes.data_as(_lib.c_double_p)
        self.kT, self.seeds = kT.copy(), seeds.copy()
        self.system = system
        _lib.Handle.__init__(self, "mythos_martini_langevin_create_ensemble", system._h, self.n_rep, float(dt),
                             kT.ctypes.data_as(_lib.c_double_p), float(gamma), mptr, seeds.ctypes.data_as(C.POINTER(C.c_uint64)))

    def _boxes(self, box) -> np.ndarray:
        return MartiniEnsembleIntegrator.replica_boxes(box, self.n_rep)

    _replicas = property(lambda self: self.n_rep)

    def _lead(self) -> tuple:
        return (self.n_rep,)

    def restart(self, seeds, step: int = 0) -> None:
        """Make the handle new for another run (mythos_martini_langevin_restart): one seed per replica, the step counter set,
        the resident state dropped - ``load`` or ``run`` comes next.  Settings and buffers stay; the exchange ladder goes
        back to the identity and the exchange counts to zero."""
        sd = np.ascontiguousarray(np.asarray([int(x) & (2**64 - 1) for x in seeds], dtype=np.uint64))
        if sd.shape != (self.n_rep,):
            raise ValueError(f"seeds must hold {self.n_rep} values, one per replica")
        _lib.check(self._lib.mythos_martini_langevin_restart(self._h, sd.ctypes.data_as(C.POINTER(C.c_uint64)), int(step)), "restart")
        self.seeds = sd.copy()

    # ---- what the two exchanges' readers share: `name` is the C entry point behind "mythos_martini_langevin_" ----
    def _permutation(self, name: str) -> np.ndarray:
        a = np.zeros(self.n_rep, dtype=np.int32)
        _lib.check(getattr(self._lib, "mythos_martini_langevin_" + name)(self._h, a.ctypes.data_as(C.POINTER(C.c_int32))), name)
        return a.astype(np.int64)

    def _counted(self, name: str, width: int, dtype, ctype) -> np.ndarray:
        """The (rows, width) array behind a (handle, array or NULL, count) entry point: count, then fill."""
        fn, n = getattr(self._lib, "mythos_martini_langevin_" + name), C.c_int(0)
        _lib.check(fn(self._h, None, C.byref(n)), name)
        a = np.zeros((n.value, width), dtype=dtype)
        if n.value:
            _lib.check(fn(self._h, a.ctypes.data_as(C.POINTER(ctype)), C.byref(n)), name)
        return a

    def _last_rows(self, name: str) -> torch.Tensor:
        return torch.as_tensor(self._counted(name, self.n_rep, np.int32, C.c_int32).astype(np.int64), device=self.system.device)

    def _last_log(self, name: str, fields: tuple) -> dict:
        rec = self._counted(name, len(fields), np.float64, C.c_double)
        out = {k: rec[:, j].copy() for j, k in enumerate(fields)}
        for k in ("step", "rung", "slot_a", "slot_b"):
            out[k] = out[k].astype(np.int64)
        out["accepted"] = out["accepted"] != 0.0
        return out

    def _counts(self, name: str) -> tuple[np.ndarray, np.ndarray]:
        att, acc = np.zeros(self.n_rep - 1, dtype=np.int64), np.zeros(self.n_rep - 1, dtype=np.int64)
        _lib.check(getattr(self._lib, "mythos_martini_langevin_" + name)(self._h, att.ctypes.data_as(C.POINTER(C.c_int64)),
                                                                         acc.ctypes.data_as(C.POINTER(C.c_int64))), name)
        return att, acc

    # ---- replica exchange between the temperatures (mythos_martini_langevin_set_exchange, include/mythos_hip.h) ----
    EXCHANGE_FIELDS = ("step", "rung", "slot_a", "slot_b", "u_a", "u_b", "v_a", "v_b", "d", "u", "accepted")

    def set_exchange(self, every: int, seed: int = 0) -> None:
        """An exchange event at every absolute step s > 0 with s % ``every`` == 0 (0: off); ``seed`` keys the decisions'
        uniforms.  Handles with at least two replicas."""
        _lib.check(self._lib.mythos_martini_langevin_set_exchange(self._h, int(every), int(seed) & (2**64 - 1)), "set_exchange")

    @staticmethod
    def _ladder_arg(rung_of_slot) -> np.ndarray:
        return np.ascontiguousarray(np.asarray(rung_of_slot, dtype=np.int64).reshape(-1), dtype=np.int32)

    def set_ladder(self, rung_of_slot) -> None:
        """Which rung of the ladder - the ``kT`` of creation, in their order - every slot runs at: a permutation of
        0 .. R - 1.  Rewrites the slots' kT; refused while the resident frame is open."""
        a = self._ladder_arg(rung_of_slot)
        if a.shape != (self.n_rep,):
            raise ValueError(f"rung_of_slot must hold {self.n_rep} values, one per replica")
        _lib.check(self._lib.mythos_martini_langevin_set_ladder(self._h, a.ctypes.data_as(C.POINTER(C.c_int32))), "set_ladder")

    @property
    def ladder(self) -> np.ndarray:
        """(R,) int64: ``rung_of_slot`` of the resident state."""
        return self._permutation("get_ladder")

    @property
    def kT_now(self) -> np.ndarray:
        """(R,) float64: the kT every slot runs at now."""
        return self.kT[self.ladder]

    @property
    def last_ladder(self) -> torch.Tensor:
        """(S, R) int64 on the system's device: ``rung_of_slot`` at every row the last call saved, each before the events of
        its step."""
        return self._last_rows("last_ladder")

    @property
    def last_exchanges(self) -> dict:
        """The last call's attempts in order, a dict of (A,) arrays: ``step``, ``rung`` (the pair is rung, rung + 1),
        ``slot_a``, ``slot_b`` int64; ``u_a``, ``u_b`` (kJ/mol), ``v_a``, ``v_b`` (nm^3), ``d``, ``u`` float64; ``accepted``
        bool."""
        return self._last_log("last_exchanges", self.EXCHANGE_FIELDS)

    def exchange_counts(self) -> tuple[np.ndarray, np.ndarray]:
        """(attempts, accepts), (R - 1,) int64 each: per rung pair (t, t + 1) since ``restart``."""
        return self._counts("exchange_counts")

    # ---- window exchange between the rows of the installed restraints (mythos_martini_langevin_set_window_exchange) ----
    WINDOW_EXCHANGE_FIELDS = ("step", "rung", "slot_a", "slot_b", "e_t_a", "e_t1_a", "e_t_b", "e_t1_b", "d", "u", "accepted")

    def set_window_exchange(self, every: int, seed: int = 0) -> None:
        """A window-exchange event at every absolute step s > 0 with s % ``every`` == 0 (0: off); ``seed`` keys the
        decisions' uniforms.  Every replica at the same kT; refused together with temperature exchange or a barostat."""
        _lib.check(self._lib.mythos_martini_langevin_set_window_exchange(self._h, int(every), int(seed) & (2**64 - 1)), "set_window_exchange")

    def set_windows(self, window_of_slot) -> None:
        """Which window - the parameter row ``set_restraints`` was given for that replica - every slot holds: a permutation
        of 0 .. R - 1.  Moves the rows on the device; refused while the resident frame is open."""
        a = self._ladder_arg(window_of_slot)
        if a.shape != (self.n_rep,):
            raise ValueError(f"window_of_slot must hold {self.n_rep} values, one per replica")
        _lib.check(self._lib.mythos_martini_langevin_set_windows(self._h, a.ctypes.data_as(C.POINTER(C.c_int32))), "set_windows")

    @property
    def windows(self) -> np.ndarray:
        """(R,) int64: ``window_of_slot`` of the resident state."""
        return self._permutation("get_windows")

    @property
    def last_windows(self) -> torch.Tensor:
        """(S, R) int64 on the system's device: ``window_of_slot`` at every row the last call saved, each before the event
        of its step."""
        return self._last_rows("last_windows")

    @property
    def last_window_exchanges(self) -> dict:
        """The last call's attempts in order, a dict of (A,) arrays: ``step``, ``rung`` (the pair is rung, rung + 1),
        ``slot_a``, ``slot_b`` int64; ``e_t_a``, ``e_t1_a``, ``e_t_b``, ``e_t1_b`` (kJ/mol: the restraint energy of slot
        A's / slot B's configuration under window rung / rung + 1), ``d``, ``u`` float64; ``accepted`` bool."""
        return self._last_log("last_window_exchanges", self.WINDOW_EXCHANGE_FIELDS)

    def window_exchange_counts(self) -> tuple[np.ndarray, np.ndarray]:
        """(attempts, accepts), (R - 1,) int64 each: per rung pair (t, t + 1) since ``set_restraints``."""
        return self._counts("window_exchange_counts")

    def pressure(self) -> dict:
        """As :meth:`MartiniLangevinIntegrator.pressure`, per replica: ``kinetic``, ``virial``, ``pressure`` (R, 3),
        ``volume`` and ``p`` (R,)."""
        out = np.zeros((self.n_rep, 10), dtype=np.float64)
        _lib.check(self._lib.mythos_martini_langevin_pressure_ensemble(self._h, out.ctypes.data_as(_lib.c_double_p),
                                                                       _lib.stream(self.system.device)), "martini_langevin_pressure")
        return {"kinetic": out[:, 0:3].copy(), "virial": out[:, 3:6].copy(), "pressure": out[:, 6:9].copy(), "volume": out[:, 9].copy(),
                "p": out[:, 6:9].mean(axis=1)}

    @property
    def box(self) -> np.ndarray:
        """(R, 3) float64: every replica's box of the resident state."""
        b = np.zeros((self.n_rep, 3), dtype=np.float64)
        _lib.check(self._lib.mythos_martini_langevin_get_box_ensemble(self._h, b.ctypes.data_as(_lib.c_double_p)), "get_box")
        return b

    @property
    def last_boxes(self) -> torch.Tensor:
        """(S, R, 3) float64 on the system's device: every replica's box at every row the last call saved."""
        n = C.c_int(0)
        _lib.check(self._lib.mythos_martini_langevin_last_boxes(self._h, None, C.byref(n)), "last_boxes")
        b = np.zeros((n.value, self.n_rep, 3), dtype=np.float64)
        if n.value:
            _lib.check(self._lib.mythos_martini_langevin_last_boxes(self._h, b.ctypes.data_as(_lib.c_double_p), C.byref(n)), "last_boxes")
        return torch.as_tensor(b, device=self.system.device)

    def init_velocities(self) -> torch.Tensor:
        """(R, n, 3): replica r's are those a single integrator with ``seeds[r]`` and ``kT[r]`` draws."""
        v = torch.empty((self.n_rep, self.system.n, 3), dtype=self.system.dtype, device=self.system.device)
        _lib.check(self._lib.mythos_martini_langevin_init_velocities(self._h, _lib.ptr(v), _lib.stream(self.system.device)), "init_velocities")
        return v

    def _check_state(self, pos, vel):
        s = self.system
        shape = (self.n_rep, s.n, 3)
        for t, name in ((pos, "pos"), (vel, "vel")):
            if t.device != s.device or t.dtype != s.dtype or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous {s.dtype} tensor of shape {shape} on {s.device}")

    def _rows(self, n_steps: int, save_every: int, want_energy: bool):
        s = self.system
        ns = n_steps // save_every if save_every > 0 else 0
        traj = torch.empty((ns, self.n_rep, s.n, 3), dtype=s.dtype, device=s.device) if ns else None
        et = torch.zeros((ns, self.n_rep, 5 if s.charged else 4), dtype=torch.float64, device=s.device) if (ns and want_energy) else None
        return traj, et

    def run(self, pos, vel, box, n_steps: int, save_every: int = 0, want_energy: bool = True):
        """Advance ``pos`` / ``vel`` (R, n, 3) in place -> (traj (S, R, n, 3) or None, e_trace (S, R, 4 | 5) or None)."""
        self._check_state(pos, vel)
        box = self._boxes(box)
        traj, et = self._rows(n_steps, save_every, want_energy)
        rc = self._lib.mythos_martini_langevin_run(
            self._h, _lib.ptr(pos), _lib.ptr(vel), box.ctypes.data_as(_lib.c_double_p), int(n_steps), int(save_every),
            _lib.ptr(traj), _lib.ptr(et), _lib.stream(self.system.device))
        _touched(pos, vel)
        _lib.check(rc, "martini_langevin_run")
        return traj, et

    def load(self, pos, vel, box) -> None:
        self._check_state(pos, vel)
        box = self._boxes(box)
        _lib.check(self._lib.mythos_martini_langevin_load(self._h, _lib.ptr(pos), _lib.ptr(vel), box.ctypes.data_as(_lib.c_double_p),
                                                          _lib.stream(self.system.device)), "martini_langevin_load")

    def rows(self, pruned: bool = False):
        """(rows (R n, stride) int32 of bead indices inside the replica, lengths (R n,) int32), replica-major."""
        stride = C.c_int(0)
        which = 1 if pruned else 0
        _lib.check(self._lib.mythos_martini_langevin_get_rows(self._h, which, None, None, C.byref(stride)), "get_rows")
        rows = np.empty((self.n_rep * self.system.n, stride.value), dtype=np.int32)
        lens = np.empty(self.n_rep * self.system.n, dtype=np.int32)
        _lib.check(self._lib.mythos_martini_langevin_get_rows(self._h, which, rows.ctypes.data_as(C.POINTER(C.c_int32)),
                                                              lens.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(stride)), "get_rows")
        return rows, lens


class MartiniEnsembleIntegrator:
    """R independent copies ("replicas") of one :class:`MartiniSystem`, each with its own ``kT``, box, seed and - when a
    barostat is set - coupling history, advanced by ONE step launch per time step
    (mythos_martini_langevin_create_ensemble).  Stands in for the reference's loop over simulation temperatures, one
    GROMACS run each (examples/scripts/martini_full_reparameterization.py:347-357).

    The methods are those of :class:`MartiniLangevinIntegrator` with a leading replica axis on every tensor: ``pos`` /
    ``vel`` (R, n, 3), ``box`` (R, 3) or (3,) for all, ``traj`` (rows, R, n, 3), ``e_trace`` (rows, R, 4 | 5),
    ``last_boxes`` (rows, R, 3), ``pressure()`` a dict of (R, ...) arrays, ``rows()`` over the R n rows (local bead
    indices).  Neighbour policy, pruned rows, barostat settings and timing apply to all replicas alike.  Replica r is bit
    for bit the single integrator made with ``kT[r]``, ``seeds[r]`` and loaded with ``box[r]`` while no call reports a
    recovery - between exchange events, with the slot's current kT.  ``seeds``: one per replica, an int s for s + r,
    None for 0 + r.

    Replica exchange between the temperatures (``set_exchange(every, seed)``; the rule is in include/mythos_hip.h): the
    replicas are *slots* that keep their beads, box and seed, ``kT`` is the ladder of *rungs*, and an accepted exchange
    swaps the kT of two slots and rescales their velocities.  ``ladder`` / ``set_ladder`` give and take ``rung_of_slot``,
    ``kT_now`` the slots' current kT, ``last_ladder`` (rows, R) the ladder at every saved row, ``last_exchanges`` the log of
    the last call's attempts and ``exchange_counts()`` attempts and acceptances per rung pair since ``restart``.

    Window exchange (``set_window_exchange(every, seed)``; a mode of its own, every replica at the same kT): the rungs are
    the per-replica parameter rows of the installed restraints, and an accepted exchange swaps the rows of two slots on the
    device.  ``windows`` / ``set_windows`` give and take ``window_of_slot``, ``last_windows`` (rows, R) the assignment at
    every saved row, ``last_window_exchanges`` the log of the last call's attempts and ``window_exchange_counts()``
    attempts and acceptances per rung pair since ``set_restraints``."""

    KB = MartiniLangevinIntegrator.KB

    def __init__(self, system: MartiniSystem, dt, kT, gamma, mass=None, seeds=None):
        self._impl = _MartiniEnsembleHandle(system, dt, kT, gamma, mass=mass, seeds=seeds)

    def __getattr__(self, name):
        # everything else - set_neighbor_policy, set_inner_list, set_barostat, load, advance, run, store, pressure, box,
        # last_boxes, rows, step, the counters, close - is the handle's
        if name == "_impl":
            raise AttributeError(name)
        return getattr(self._impl, name)

    @staticmethod
    def replica_boxes(box, n_rep: int) -> np.ndarray:
        """``box`` (R, 3), or (3,) for every replica -> contiguous (R, 3) float64; anything else is refused."""
        box = np.asarray(box, dtype=np.float64)
        if box.shape == (3,):
            box = np.broadcast_to(box, (n_rep, 3))
        if box.shape != (n_rep, 3):
            raise ValueError(f"box must have shape ({n_rep}, 3), or (3,) for every replica")
        return np.ascontiguousarray(box)

    @staticmethod
    def check(n: int, kT, r_cut: float = 1.1, skin: float = 0.2, boxes=None) -> None:
        """What creation and ``load`` refuse, without a device (mythos_martini_ensemble_check): fewer than one replica, a
        kT that is not finite and positive, more rows than the neighbour store indexes, a replica box under
        2 (r_cut + skin).  Raises with the library's message."""
        kT = np.ascontiguousarray(np.atleast_1d(np.asarray(kT, dtype=np.float64)))
        b = None if boxes is None else MartiniEnsembleIntegrator.replica_boxes(boxes, int(kT.size))
        _lib.check(_lib.load().mythos_martini_ensemble_check(
            int(n), int(kT.size), kT.ctypes.data_as(_lib.c_double_p), float(r_cut), float(skin),
            None if b is None else b.ctypes.data_as(_lib.c_double_p)), "martini_ensemble_check")

    @staticmethod
    def check_exchange(n_rep: int, every: int = 0, rung_of_slot=None) -> None:
        """What ``set_exchange`` and ``set_ladder`` refuse, without a device (mythos_martini_exchange_check): fewer than two
        replicas, ``every`` < 0, a ``rung_of_slot`` of ``n_rep`` entries that is no permutation.  Raises with the library's message."""
        a = None
        if rung_of_slot is not None:
            a = _MartiniEnsembleHandle._ladder_arg(rung_of_slot)
            if a.shape != (int(n_rep),):
                raise ValueError(f"rung_of_slot must hold {int(n_rep)} values, one per replica")
        _lib.check(_lib.load().mythos_martini_exchange_check(int(n_rep), int(every), None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))),
                   "martini_exchange_check")

    @staticmethod
    def check_window_exchange(n_rep: int, every: int = 0, kT=None, temperature_exchange: bool = False, barostat: bool = False,
                              p_param=None, window_of_slot=None) -> None:
        """What ``set_window_exchange``, ``set_windows`` and ``set_restraints`` under window exchange refuse, without a device
        (mythos_martini_window_exchange_check): fewer than two replicas, ``every`` < 0, replicas whose ``kT`` differ,
        temperature exchange or a barostat beside it, ``p_param`` (R, P, 9) of a lowered set whose vec or origin differ
        between replicas, a ``window_of_slot`` that is no permutation.  Raises with the library's message."""
        n_rep = int(n_rep)
        k = None
        if kT is not None:
            k = np.ascontiguousarray(np.asarray(kT, dtype=np.float64).reshape(-1))
            if k.shape != (n_rep,):
                raise ValueError(f"kT must hold {n_rep} values, one per replica")
        q, n_pull = None, 0
        if p_param is not None:
            q = np.ascontiguousarray(p_param, dtype=np.float64)
            if q.ndim != 3 or q.shape[0] != n_rep or q.shape[2] != 9:
                raise ValueError(f"p_param must have shape ({n_rep}, P, 9)")
            n_pull = int(q.shape[1])
        a = None
        if window_of_slot is not None:
            a = _MartiniEnsembleHandle._ladder_arg(window_of_slot)
            if a.shape != (n_rep,):
                raise ValueError(f"window_of_slot must hold {n_rep} values, one per replica")
        _lib.check(_lib.load().mythos_martini_window_exchange_check(
            n_rep, int(every), None if k is None else k.ctypes.data_as(_lib.c_double_p), int(bool(temperature_exchange)), int(bool(barostat)),
            n_pull, None if q is None else q.ctypes.data_as(_lib.c_double_p), None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))),
            "martini_window_exchange_check")
