"""oxDNA's energy file, with the order parameters and umbrella weights of an umbrella-sampling run.

Mirrors ``read_energy`` of mythos/simulators/oxdna/utils.py:348-384 (and the part of mythos/input/oxdna_input.py it needs:
the ``key = value`` lines of an oxDNA ``input`` file).  Columns as numpy arrays instead of a pandas frame.
"""

from __future__ import annotations

from pathlib import Path

import numpy as np

BASE_COLUMNS = ("time", "potential_energy", "acc_ratio_trans", "acc_ratio_rot", "acc_ratio_vol")


def read_input(path) -> dict[str, str]:
    """``key = value`` lines of an oxDNA input file as strings; ``#`` comments, blank lines and the braces of nested
    blocks are skipped."""
    out = {}
    for line in Path(path).read_text().splitlines():
        line = line.split("#", 1)[0].strip()
        if not line or "=" not in line:
            continue
        key, value = line.split("=", 1)
        out[key.strip()] = value.strip()
    return out


def order_parameter_names(op_file) -> list[str]:
    """The ``order_parameter = ...`` of every block of an order-parameter file, in file order."""
    return [line.split("=", 1)[1].strip() for line in Path(op_file).read_text().splitlines()
            if line.strip().startswith("order_parameter")]


def _truthy(value: str | None) -> bool:
    return value is not None and value.strip().lower() not in ("", "0", "false", "no")


def read_energy(simulation_dir) -> dict[str, np.ndarray]:
    """Columns of the energy file of the oxDNA run in ``simulation_dir`` (its ``input`` names the file).  The first row -
    step 0, which the trajectory file does not hold - is dropped, so row k belongs to configuration k of the trajectory.
    ``time, potential_energy, acc_ratio_trans, acc_ratio_rot, acc_ratio_vol``; under ``umbrella_sampling`` then one column
    per order parameter of the ``op_file`` (named after its ``order_parameter``) and ``weight``."""
    simulation_dir = Path(simulation_dir)
    inputs = read_input(simulation_dir / "input")
    columns = list(BASE_COLUMNS)
    if _truthy(inputs.get("umbrella_sampling")):
        columns += order_parameter_names(simulation_dir / inputs["op_file"]) + ["weight"]
    rows = np.loadtxt(simulation_dir / inputs["energy_file"], dtype=np.float64, skiprows=1, ndmin=2)
    if rows.shape[1] != len(columns):
        raise ValueError(f"{inputs['energy_file']} has {rows.shape[1]} columns, the input file describes {len(columns)}: {columns}")
    return {name: rows[:, k].copy() for k, name in enumerate(columns)}
