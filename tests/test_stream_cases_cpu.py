"""Every export of include/mythos_hip.h that takes a stream, sets a table or reads one back has a stream case in
tests/test_gpu_streams.py, and the header says what it does with the stream: an export cannot arrive without either.

Parsed from the header: the prototypes, and for each the comment in front of it (the nearest one; prototypes that follow
one comment share it) with a comment on its own line behind the semicolon.  Needs no GPU."""

from __future__ import annotations

import re
from pathlib import Path

from tests import stream_order as SO
from tests import test_gpu_streams as T

HEADER = Path(__file__).resolve().parent.parent / "include" / "mythos_hip.h"
EXEMPT = re.compile(r"(_check|_create|_destroy|_count|_name|_width)$|_n_")
STATEFUL = re.compile(r"_set_|_get_|_last_|_stats$|_counts$|_restart$")
WORDS = ("asynchronous", "synchronis", "waits")


def parse_header(text: str) -> dict:
    """{export: (has a mythos_stream_t parameter, its comment)} of every prototype."""
    out = {}
    pieces = re.split(r"(/\*.*?\*/)", text, flags=re.S)
    last_comment = ""
    for k, piece in enumerate(pieces):
        if piece.startswith("/*"):
            # a comment right behind a semicolon on the same line belongs to the prototype in front of it
            before = pieces[k - 1] if k else ""
            if re.search(r";[ \t]*\Z", before) and out:
                name = list(out)[-1]
                out[name] = (out[name][0], out[name][1] + " " + piece)
            else:
                last_comment = piece
            continue
        for m in re.finditer(r"\b(mythos_\w+)\s*\(([^;{}]*?)\)\s*;", piece, flags=re.S):
            if "typedef" in piece[max(0, m.start() - 40):m.start()].split(";")[-1]:
                continue
            out[m.group(1)] = ("mythos_stream_t" in m.group(2), last_comment)
    return out


EXPORTS = parse_header(HEADER.read_text())


def _covered() -> dict:
    cov = {}
    for case in [*T.CASES, *T.SET_CASES]:
        for name, kinds in case.covers.items():
            assert set(kinds) <= {SO.IN, SO.OUT, SO.SET, SO.GET} and kinds, (case.name, name, kinds)
            cov.setdefault(name, set()).update(kinds)
    return cov


def test_the_header_was_parsed():
    assert len(EXPORTS) > 130
    assert EXPORTS["mythos_oxdna_energy"][0] and not EXPORTS["mythos_oxdna_set_params"][0]
    assert "Replaces with_params" in EXPORTS["mythos_oxdna_set_params"][1] or "replaces with_params" in EXPORTS["mythos_oxdna_set_params"][1]
    assert "mythos_langevin_store" in EXPORTS and "mythos_mbar_boot_binned" in EXPORTS


def test_the_cases_name_real_exports_and_excuse_none_they_cover():
    cov = _covered()
    assert not set(cov) - set(EXPORTS), sorted(set(cov) - set(EXPORTS))
    assert not set(T.EXCLUDED) - set(EXPORTS), sorted(set(T.EXCLUDED) - set(EXPORTS))
    assert not set(T.EXCLUDED) & set(cov), sorted(set(T.EXCLUDED) & set(cov))
    assert all(len(reason) > 20 for reason in T.EXCLUDED.values())


def test_every_export_with_a_stream_has_an_in_or_out_case():
    cov = _covered()
    missing = [n for n, (has_stream, _) in EXPORTS.items() if has_stream and not ({SO.IN, SO.OUT} & cov.get(n, set()))]
    assert not missing, missing  # (a stream entry is never excused)


def test_every_setter_and_getter_has_a_case_or_a_reason():
    cov = _covered()
    matching = [n for n, (has_stream, _) in EXPORTS.items() if (has_stream or STATEFUL.search(n)) and not (EXEMPT.search(n) and not has_stream)]
    missing = [n for n in matching if n not in cov and n not in T.EXCLUDED]
    assert not missing, missing
    excused = [n for n in matching if n in T.EXCLUDED]
    assert len(excused) <= 0.10 * len(matching), (len(excused), len(matching))


def test_the_header_states_the_stream_contract_of_every_covered_entry():
    silent = sorted(n for n in _covered() if not any(w in EXPORTS[n][1].lower() for w in WORDS))
    assert silent == sorted(T.UNDOCUMENTED), silent
    assert T.UNDOCUMENTED == []


def test_every_case_states_where_its_delay_must_be_pending():
    """(statically: the call of every case uses the probe; the GPU tests assert that it fired)"""
    import inspect

    for case in [*T.CASES, *T.SET_CASES]:
        src = inspect.getsource(case.call)
        assert "probe.after()" in src or "probe.before()" in src, case.name
