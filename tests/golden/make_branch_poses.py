"""Regenerate the branch-pose fixtures tests/golden/branch_poses/model{1,2,3}.dat.

Seeded draws around the ideal geometry of every pair term, evaluated with the oracle and selected per branch cell
(tests/oxdna_branch_poses.py build_poses).  Deterministic: a second run writes the same bytes.  Run from the repository root:

    python tests/golden/make_branch_poses.py
"""

import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

from tests import oxdna_branch_poses as BP  # noqa: E402


def main() -> None:
    BP.FIXTURE_DIR.mkdir(exist_ok=True)
    for model in BP.MODELS:
        poses = BP.build_poses(model)
        BP.fixture_path(model).write_text(BP.fixture_text(poses))
        BP.load_fixture.cache_clear()
        rows, text = BP.cell_table(BP.load_fixture(model))
        print(text)
        short = [c for c, n, w in rows if n < BP.K_LIVE]
        print(f"model {model}: {poses.n} poses, {len(rows)} reachable cells, {len(short)} below {BP.K_LIVE} live poses: {short}")


if __name__ == "__main__":
    main()
