"""Provenance of ``tests/golden/melting_temp/``: the umbrella-sampling run the reference ships for its melting-temperature
test (``data/test-data/melting_temp/``: a 12-nt oxDNA1 duplex, VMMC at 307.15 K, 1000 printed configurations with the
``bond`` and ``mindistance`` order parameters and the umbrella weight of every one in ``energy.dat``).  DATA files only.

    python tests/golden/copy_melting_fixtures.py            # copies and verifies
    python tests/golden/copy_melting_fixtures.py --check    # only verifies

``sys.top``, ``input``, ``op.txt`` and ``last_hist.dat`` are byte copies.  The trajectory (2.17 MB) is over the size limit
of a committed file, so ``trajectory.dat.gz`` holds its first FRAMES configurations (gzip of the byte prefix, 0.83 MB of
text: kept compressed so that the fixture does not swamp a diff) and ``energy.dat`` the matching FRAMES + 1 lines (oxDNA
prints step 0 to the energy file and not to the trajectory); a trimmed file is checked to be a prefix of the reference's.
FRAMES = 384: the melting curve of the first 384 configurations crosses 0.5 inside the 280 K - 350 K range (229 of them
are unbound); up to 128 it never does and the melting temperature pins to the range's edge.
"""

import argparse
import filecmp
import gzip
import shutil
from pathlib import Path

REF = Path("/root/reference/data/test-data/melting_temp")
DST = Path(__file__).resolve().parent / "melting_temp"

COPIES = ("sys.top", "input", "op.txt", "last_hist.dat")
FRAMES = 384
LINES_PER_FRAME = 3 + 12  # "t =", "b =", "E =" and one line per nucleotide
TRIMMED = {"trajectory.dat": FRAMES * LINES_PER_FRAME, "energy.dat": FRAMES + 1}
GZIPPED = ("trajectory.dat",)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    bad = 0
    if not args.check:
        DST.mkdir(parents=True, exist_ok=True)
    for name in COPIES:
        if not args.check:
            shutil.copyfile(REF / name, DST / name)
        if not (DST / name).exists() or not filecmp.cmp(REF / name, DST / name, shallow=False):
            print("MISMATCH", name)
            bad += 1
    for name, n_lines in TRIMMED.items():
        whole = (REF / name).read_bytes()
        head = b"".join(whole.splitlines(keepends=True)[:n_lines])
        dst = DST / (name + ".gz" if name in GZIPPED else name)
        if not args.check:
            dst.write_bytes(gzip.compress(head, 9, mtime=0) if name in GZIPPED else head)
        got = None
        if dst.exists():
            got = gzip.decompress(dst.read_bytes()) if name in GZIPPED else dst.read_bytes()
        if got != head or not whole.startswith(head) or head.count(b"\n") != n_lines:
            print("MISMATCH (trimmed)", name)
            bad += 1
    print("ok" if bad == 0 else f"{bad} file(s) differ")
    raise SystemExit(1 if bad else 0)


if __name__ == "__main__":
    main()
