"""From energy functions to kernel inputs: the one place that knows how a composed energy function becomes the model
number, the flat parameter vector, the term weights, the topology arrays and the sequence tables a system handle takes.
``ComposedEnergyFunction._evaluate`` and ``HipMDSimulator._prepare`` both start here, so an energy call and a simulation
of the same function see the same parameters and refuse the same malformed compositions.
"""

from __future__ import annotations

import dataclasses as dc
from typing import Any

import numpy as np
import torch

from mythos_amd import _lib
from mythos_amd.energy import flat_params as fp
from mythos_amd.energy import terms as _terms
from mythos_amd.energy.base import TERM_ORDER, pseq_request
from mythos_amd.input.topology import NucleotideType


def _np(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    return np.asarray(x)


@dc.dataclass(frozen=True)
class Lowered:
    model: int  # of the C ABI: 1 dna1, 2 dna2, 3 rna2, 4 na1
    flat: torch.Tensor  # fp64, with the autograd graph of the parameters; oxNA: the oxDNA2 | oxRNA2 | hybrid vectors
    term_weights: list  # 8, in kernel column order (TERM_ORDER); 0 for a term the function does not carry
    cols: list  # kernel column of each composed function
    seq: np.ndarray
    is_end: np.ndarray | None
    bonded: np.ndarray
    unbonded: Any  # as the first function carries it: (P, 2) or (2, P)
    is_rna: np.ndarray | None  # oxNA only
    box: np.ndarray | None
    pseq: tuple | None  # pseq_request: (marginals, unit, bp_probs, terms)
    # what the flat vector was derived from (a temperature sweep derives its kT-dependent entries again, map_kt)
    sections: dict | None = None  # derive_flat's sections, defaults filled in; None for oxNA (three sets)
    kt: Any = None  # of a section that carries none of its own
    salt_conc: Any = None


def lower(energy_fns, weights, *, kt_default=None) -> Lowered:
    """``kt_default``: the temperature of a function none of whose terms carries ``kt`` (a simulator passes its own kT;
    an energy call leaves it to the model's default)."""
    if not energy_fns:
        raise ValueError("ComposedEnergyFunction has no energy functions")
    geom = next((fn.transform_fn for fn in energy_fns if fn.transform_fn is not None), None)
    if geom is None:
        raise ValueError("transform_fn (site geometry) must be provided")
    model = geom.model  # the site geometry decides oxDNA1 vs oxDNA2 (shared term classes exist in both)
    _terms.check_term_models(model, energy_fns)
    na1 = model == 4
    # oxNA (mythos/energy/na1/): every term carries three parameter sets - oxDNA2, oxRNA2, hybrid - and the nucleotide types
    sets = {which: {"geometry": geom.params[which]} if which in geom.params else {} for which in fp.NA1_SETS} if na1 else None
    sections = None if na1 else {"geometry": geom.params}
    term_w, cols = [0.0] * 8, []
    w_user = weights if weights is not None else torch.ones(len(energy_fns), dtype=torch.float64)
    kt = salt = hce = nt_type = None
    for fn, w in zip(energy_fns, w_user):
        k = TERM_ORDER.index(fn.term)
        if k in cols:
            raise ValueError(f"term '{fn.term}' appears twice in one composed energy function")
        if na1:
            for which, sec in fn.params.sections().items():
                sets[which][fn.term] = sec
            t = np.asarray(_np(fn.params["nt_type"]))
            if nt_type is not None and not np.array_equal(nt_type, t):
                raise ValueError("the terms of an oxNA energy function carry different nt_type arrays")
            nt_type = t
        else:
            sections[fn.term] = {n: fn.params[n] for n in (*type(fn.params).required_params, *type(fn.params).optional_params)
                                 if n not in ("pseq", "pseq_constraints")}  # the sequence distribution is not a flat parameter
        term_w[k] = float(w)
        cols.append(k)
        if "kt" in fn.params and kt is None:
            kt = fn.params["kt"]
        if fn.term == "debye":
            salt, hce = fn.params["salt_conc"], bool(fn.params["half_charged_ends"])
    if kt is None:
        kt = _terms.default_kt() if kt_default is None else kt_default
    kw = dict(kt=kt, salt_conc=0.5 if salt is None else salt, term_weights=term_w, numbers_ok=True)
    first = energy_fns[0]
    seq = _np(first.seq)
    if na1:
        _terms.fill_missing_sections_na1(sets)
        named = fp.derive_flat_na1(sets["dna"], sets["rna"], sets["drh"], half_charged_ends=False if hce is None else hce, **kw)
        flat = fp.pack_flat_na1(named, _lib.param_names())
        if nt_type.shape != (int(seq.shape[0]),):
            raise ValueError("nt_type must have one entry per nucleotide")
    else:
        _terms.fill_missing_sections(model, sections)
        flat = fp.pack_flat(fp.derive_flat(model, sections, half_charged_ends=True if hce is None else hce, **kw), _lib.param_names())
    return Lowered(model=model, flat=flat, term_weights=term_w, cols=cols, seq=seq,
                   is_end=None if first.is_end is None else _np(first.is_end), bonded=_np(first.bonded_neighbors),
                   unbonded=first.unbonded_neighbors, is_rna=nt_type == int(NucleotideType.RNA) if na1 else None,
                   box=getattr(first.displacement_fn, "box", None), pseq=pseq_request(energy_fns), sections=sections, kt=kt,
                   salt_conc=kw["salt_conc"])
