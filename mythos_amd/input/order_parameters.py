"""oxDNA's order-parameter file and umbrella weights file.

An order-parameter file (``op_file`` of an oxDNA input) is a sequence of brace blocks::

    {
        order_parameter = bond
        name = all_native_bonds
        pair1 = 0, 11
        pair2 = 1, 10
    }
    {
        order_parameter = mindistance
        name = dist
        pair1 = 0, 11
        interfaces = 1.0, 2.0, 4.0
    }

Every file the reference ships uses these two kinds.  The weights file (``weights_file``) has one row per state of
the order parameters, ``state_1 ... state_k weight``, in any order.
"""

from __future__ import annotations

import dataclasses as dc
import re
from pathlib import Path

import numpy as np

KINDS = ("bond", "mindistance")  # in the order of MYTHOS_OP_BOND, MYTHOS_OP_MINDISTANCE (include/mythos_hip.h)


@dc.dataclass(frozen=True)
class OrderParameter:
    """One block of an order-parameter file.  ``pairs``: tuple of (i, j) nucleotide indices; ``interfaces``: the
    boundaries between the states of a ``mindistance`` parameter, () for ``bond``."""

    kind: str
    name: str
    pairs: tuple
    interfaces: tuple = ()

    def __post_init__(self):
        if self.kind not in KINDS:
            raise ValueError(f"order_parameter = {self.kind}: only {' and '.join(KINDS)} are built")
        pairs = tuple((int(i), int(j)) for i, j in self.pairs)
        if not pairs:
            raise ValueError(f"order parameter '{self.name}' lists no pair")
        for i, j in pairs:
            if i == j:
                raise ValueError(f"order parameter '{self.name}' pairs nucleotide {i} with itself")
            if i < 0 or j < 0:
                raise ValueError(f"order parameter '{self.name}' has a negative nucleotide index")
        interfaces = tuple(float(x) for x in self.interfaces)
        if self.kind == "mindistance" and not interfaces:
            raise ValueError(f"mindistance order parameter '{self.name}' has no interfaces")
        object.__setattr__(self, "pairs", pairs)
        object.__setattr__(self, "interfaces", interfaces)


_PAIR_KEY = re.compile(r"pair\d*$")


def read_order_parameters(path) -> tuple[OrderParameter, ...]:
    """The blocks of an oxDNA order-parameter file, in file order.  ``key = value`` with or without spaces around
    ``=``; ``#`` starts a comment; blank lines are skipped."""
    ops, block = [], None
    for no, raw in enumerate(Path(path).read_text().splitlines(), 1):
        line = raw.split("#", 1)[0].strip()
        while line:
            if line[0] == "{":
                if block is not None:
                    raise ValueError(f"{path}:{no}: '{{' inside a block")
                block, line = {"pairs": []}, line[1:].strip()
            elif line[0] == "}":
                if block is None:
                    raise ValueError(f"{path}:{no}: '}}' without a block")
                if "order_parameter" not in block:
                    raise ValueError(f"{path}:{no}: a block without 'order_parameter = ...'")
                ops.append(OrderParameter(kind=block["order_parameter"], name=block.get("name", f"op{len(ops)}"),
                                          pairs=block["pairs"], interfaces=block.get("interfaces", ())))
                block, line = None, line[1:].strip()
            else:
                body, brace, rest = line.partition("}")
                if block is None or "=" not in body:
                    raise ValueError(f"{path}:{no}: expected 'key = value' inside a block, got '{body.strip()}'")
                key, value = (s.strip() for s in body.split("=", 1))
                if _PAIR_KEY.match(key):
                    ij = [s for s in re.split(r"[,\s]+", value) if s]
                    if len(ij) != 2:
                        raise ValueError(f"{path}:{no}: a pair is two nucleotide indices, got '{value}'")
                    block["pairs"].append((int(ij[0]), int(ij[1])))
                elif key == "interfaces":
                    block["interfaces"] = tuple(float(s) for s in re.split(r"[,\s]+", value) if s)
                else:
                    block[key] = value
                line = brace + rest
    if block is not None:
        raise ValueError(f"{path}: the last block is not closed")
    return tuple(ops)


def _rows(table):
    """(state tuple, weight) rows of a weights table: a dict {state tuple (or int): weight}, or an array with one axis
    per order parameter whose entry [s_1, ..., s_k] is the weight of that state (absent states: 0)."""
    if isinstance(table, dict):
        return [((int(s),) if np.ndim(s) == 0 else tuple(int(x) for x in s), float(w)) for s, w in table.items()]
    arr = np.asarray(table, dtype=np.float64)
    if arr.ndim == 0:
        raise ValueError("a weights table has one axis per order parameter")
    return [(tuple(int(x) for x in idx), float(arr[idx])) for idx in np.ndindex(*arr.shape)]


def write_weights(path, table) -> None:
    """oxDNA's weights file: one ``state_1 ... state_k weight`` row per state of ``table`` (see ``_rows``)."""
    lines = [" ".join(str(s) for s in state) + f" {w!r}" for state, w in _rows(table)]
    Path(path).write_text("\n".join(lines) + "\n")


def read_weights(path) -> dict:
    """{(state_1, ..., state_k): weight} of an oxDNA weights file.  A state the file does not list is absent here too:
    oxDNA gives it weight 0, and a frame in it has no umbrella weight to divide by."""
    table, width = {}, None
    for no, raw in enumerate(Path(path).read_text().splitlines(), 1):
        cols = raw.split("#", 1)[0].split()
        if not cols:
            continue
        if len(cols) < 2 or (width is not None and len(cols) != width):
            raise ValueError(f"{path}:{no}: expected 'state_1 ... state_k weight' with the same k on every row")
        width = len(cols)
        state = tuple(int(s) for s in cols[:-1])
        if state in table:
            raise ValueError(f"{path}:{no}: state {state} is listed twice")
        table[state] = float(cols[-1])
    return table
