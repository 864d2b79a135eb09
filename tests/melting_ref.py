"""Oracle-side reference of the temperature sweep and of the melting temperature built on it.

Energies: the CPU oracle (``oracle/oxdna_oracle.py``) initialised anew at EVERY temperature (``orc.init_all(model, cfg,
kt=...)``) and evaluated on every frame - the definition, ``vmap(lambda kt: energy_fn.with_params(kt=kt).map(traj))``
(mythos/observables/melting_temp.py:127-140), with no knowledge of how kT enters which term.  The frames of a trajectory
are handed to ``orc.pair_terms`` as ONE system of F x N nucleotides whose pair lists are the topology's, offset per frame:
the same per-pair arithmetic, one call per temperature instead of F.
Melting temperature: the reference's formulae restated in numpy / torch without the stabilising shift of the exponent.
Gradients: torch autograd through the oracle, as the dU/dtheta tests do.
"""

from __future__ import annotations

import functools
import gzip
import tempfile
import warnings
from pathlib import Path

import numpy as np
import torch

from mythos_amd.input import defaults, oxdna_energy, topology, trajectory
from oracle import oxdna_oracle as orc
from tests import helpers as H

FIXTURE = Path(__file__).resolve().parent / "golden" / "melting_temp"
REFERENCE_RUN = Path("/root/reference/data/test-data/melting_temp")  # the full 1000-frame run, where it exists

KT_SIM = 0.10238333333333333  # 307.15 K
BOX = 20.0


def kelvin_range(lo=280.0, hi=350.0, n=20) -> np.ndarray:
    from mythos_amd.utils.units import get_kt

    return np.asarray([get_kt(t) for t in np.linspace(lo, hi, n)], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def load_run(directory: str = str(FIXTURE)):
    """(topology, trajectory, energy columns) of an oxDNA umbrella-sampling run directory."""
    base = Path(directory)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        top = topology.from_oxdna_file(base / "sys.top")
    if (base / "trajectory.dat").exists():
        traj = trajectory.from_file(base / "trajectory.dat", top.strand_counts, is_5p_3p=False)
    else:  # the fixture keeps its trajectory compressed; the reader takes a path
        with tempfile.TemporaryDirectory() as tmp:
            plain = Path(tmp) / "trajectory.dat"
            plain.write_bytes(gzip.decompress((base / "trajectory.dat.gz").read_bytes()))
            traj = trajectory.from_file(plain, top.strand_counts, is_5p_3p=False)
    return top, traj, oxdna_energy.read_energy(base)


def oracle_cfg(model: int, leaves: bool = False):
    """(sim defaults, TOML-shaped sections[, {(section, name): leaf}]) - with every non-geometry scalar a leaf that
    requires a gradient when asked."""
    sim, cfg = defaults.default_configs_for(H.model_dir(model))
    made = {}
    if leaves:
        for sec, d in cfg.items():
            if sec == "geometry":
                continue
            for k, v in list(d.items()):
                if isinstance(v, (int, float)) and not isinstance(v, bool):
                    d[k] = made[(sec, k)] = torch.tensor(float(v), dtype=torch.float64, requires_grad=True)
    return sim, cfg, made


def oracle_frame_terms(model, P, top, center, quat, box=None) -> torch.Tensor:
    """(F, n_terms) term energies of the frames center (F, N, 3), quat (F, N, 4) with the oracle parameters ``P``."""
    center, quat = torch.as_tensor(center, dtype=torch.float64), torch.as_tensor(quat, dtype=torch.float64)
    nf, n = center.shape[0], center.shape[1]
    seq, is_end, b, u = H.topo_tensors(top)
    off = (torch.arange(nf) * n)[:, None, None]
    bt, ut = orc.pair_terms(model, P, center.reshape(-1, 3), quat.reshape(-1, 4), seq.repeat(nf), is_end.repeat(nf),
                            (b[None] + off).reshape(-1, 2), (u[None] + off).reshape(-1, 2), box=box)
    names = orc.TERMS_DNA1 if model == 1 else orc.TERMS_DNA2
    both = {**bt, **ut}
    return torch.stack([both[t].reshape(nf, -1).sum(1) for t in names], dim=1)


def oracle_sweep(model, cfg, top, center, quat, kts, *, box=None, salt=0.5, hce=True, weights=None, terms=False) -> torch.Tensor:
    """(T, F) total energies (or (T, F, n_terms) with ``terms``) at every kT of ``kts``: the oracle initialised per
    temperature.  ``weights``: per-term weights of a composed function (default ones)."""
    rows = []
    for kt in kts:
        P = orc.init_all(model, cfg, kt=kt, salt_conc=salt, half_charged_ends=hce)
        e = oracle_frame_terms(model, P, top, center, quat, box)
        if not terms:
            e = e.sum(1) if weights is None else e @ torch.as_tensor(weights, dtype=torch.float64)[: e.shape[1]]
        rows.append(e)
    return torch.stack(rows)


# ---- the reference's melting-temperature formulae (mythos/observables/melting_temp.py:22-71, 130-140) ---------------------
def ref_finf(ratio):
    return 1 + 1 / (2 * ratio) - (((1 + 1 / (2 * ratio)) ** 2 - 1) ** 0.5)


def ref_ratios(e0, et, kt_sim, kts, bind_states, weights) -> torch.Tensor:
    e0, et = torch.as_tensor(e0, dtype=torch.float64), torch.as_tensor(et, dtype=torch.float64)
    kts = torch.as_tensor(np.asarray(kts), dtype=torch.float64)
    bind = torch.as_tensor(np.asarray(bind_states))
    w = torch.as_tensor(np.asarray(weights), dtype=torch.float64)
    out = []
    for t in range(et.shape[0]):
        counts = (1 / w) * torch.exp(e0 / kt_sim - et[t] / kts[t])
        out.append(ref_finf(counts[bind != 0].sum() / counts[bind == 0].sum()))
    return torch.stack(out)


def ref_interp(x: torch.Tensor, y: torch.Tensor, at: float) -> torch.Tensor:
    """y at x = ``at`` on the polyline through the points sorted by x (``jnp.interp``: constant beyond the ends)."""
    order = torch.argsort(x)
    xs, ys = x[order], y[order]
    if at <= float(xs[0].detach()):
        return ys[0]
    if at >= float(xs[-1].detach()):
        return ys[-1]
    k = int(np.searchsorted(xs.detach().numpy(), at, side="right"))
    return ys[k - 1] + (at - xs[k - 1]) / (xs[k] - xs[k - 1]) * (ys[k] - ys[k - 1])


def ref_tm(kts, ratios) -> torch.Tensor:
    return ref_interp(ratios, torch.as_tensor(np.asarray(kts), dtype=torch.float64), 0.5)


def ref_width(kts, ratios) -> torch.Tensor:
    k = torch.as_tensor(np.asarray(kts), dtype=torch.float64)
    return ref_interp(ratios, k, 0.8) - ref_interp(ratios, k, 0.2)


@functools.lru_cache(maxsize=None)
def fixture_reference(directory: str = str(FIXTURE)):
    """The oxDNA1 melting run as the reference's test sets it up (dna1 defaults, periodic box 20, sampled at KT_SIM,
    20 temperatures from 280 K to 350 K): dict of e0 (F,), et (T, F), kts, bind, weights, ratios, tm, width - numpy."""
    top, traj, en = load_run(directory)
    _, cfg, _ = oracle_cfg(1)
    kts = kelvin_range()
    box = np.full(3, BOX)
    e0 = oracle_sweep(1, cfg, top, traj.center, traj.quaternions, [KT_SIM], box=box)[0]
    et = oracle_sweep(1, cfg, top, traj.center, traj.quaternions, kts, box=box)
    ratios = ref_ratios(e0, et, KT_SIM, kts, en["bond"], en["weight"])
    return dict(e0=e0.numpy(), et=et.numpy(), kts=kts, bind=en["bond"], weights=en["weight"], ratios=ratios.numpy(),
                tm=float(ref_tm(kts, ratios)), width=float(ref_width(kts, ratios)))
