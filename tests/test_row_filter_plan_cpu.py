"""Which list rebuilds of an oxDNA run start with a wide (candidate) build: the host arithmetic of
mythos_amd/csrc/row_filter_plan.h at its boundaries, without a GPU.  The header has no HIP in it; a small program compiled
for the host walks the launches of one or more ``advance`` calls as md_drive (md_driver.h) does - a rebuild in front of
launch k once ``k - built_at >= rebuild_every``, ``since_build`` and the candidate state carried from call to call - and
prints each rebuild with the header's decision.  A wrong decision fails no parity test (every rebuild ends in a filter
that reproduces the builder's rows or halts the launches): these lines are what holds the schedule.
"""

import shutil
import subprocess

import pytest

ROOT = __import__("pathlib").Path(__file__).resolve().parents[1]
HEADER_DIR = ROOT / "mythos_amd" / "csrc"

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "row_filter_plan.h"
using namespace mythos;
// argv: rebuild_every cand_every_debug margin_debug then per call: n_launch [r<k> = a recovery in front of launch k] ...
// "load" resets the list (list_valid = false), "margin=<milli>" changes the override between calls
int main(int argc, char** argv) {
  const int every = std::atoi(argv[1]);
  const int cand_every = cand_every_for(std::atoll(argv[2]));
  long long margin_debug = std::atoll(argv[3]);
  CandState cand;
  bool list_valid = false, fitted = false;
  int since_build = 0;
  long long step = 0;
  std::printf("consts %d %d %.17g\n", kCandEvery, kCandMarginMilli, cand_stale_sq(1.0));
  for (int a = 4; a < argc; ++a) {
    const std::string_view arg(argv[a]);
    if (arg == "load") { list_valid = false, since_build = 0; continue; }
    if (arg.substr(0, 7) == "margin=") { margin_debug = std::atoll(argv[a] + 7); continue; }
    const int n_launch = std::atoi(argv[a]);
    int recover_at = -1;
    if (a + 1 < argc && argv[a + 1][0] == 'r') recover_at = std::atoi(argv[++a] + 1);
    const int milli = (int)(1e3 * cand_margin_for(margin_debug) + 0.5);
    int built_at = 0;
    auto build = [&](int k, bool recovery) {
      const bool wide = recovery || !fitted || cand_rebuild_is_wide(cand, list_valid, cand_every, milli);
      cand = cand_after(wide, cand, milli);
      std::printf("%lld %s%s\n", step + k, wide ? "wide" : "filter", recovery ? " recovery" : (list_valid ? "" : " first"));
    };
    if (!list_valid) build(0, false), fitted = true;
    else built_at = -since_build;
    list_valid = true;
    for (int k = 0; k < n_launch; ++k) {
      if (k - built_at >= every) build(k, false), built_at = k;
      if (k == recover_at) build(k, true), built_at = k, recover_at = -1;
    }
    since_build = n_launch - built_at;
    step += n_launch;
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    d = tmp_path_factory.mktemp("row_filter_plan")
    (d / "driver.cpp").write_text("#include <string_view>\n" + DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{HEADER_DIR}", str(d / "driver.cpp"), "-o", str(d / "driver")],
                   check=True, capture_output=True, text=True)

    def run(every, cand_every, margin, *calls):
        out = subprocess.run([str(d / "driver"), str(every), str(cand_every), str(margin), *map(str, calls)], check=True, capture_output=True,
                             text=True, timeout=30).stdout.splitlines()
        consts = out[0].split()
        builds = [(int(line.split()[0]), " ".join(line.split()[1:])) for line in out[1:]]
        return consts, builds

    return run


def test_the_constants_keep_the_rule(plan):
    """margin >= 1.15 * 2 * (largest centre displacement over kCandEvery intervals of 50 steps): the displacement curve of
    the 12 kbp duplex (profiles/r07_row_filter.md) in its largest window, by interval count."""
    consts, _ = plan(50, 0, 0, 1)
    every, milli, stale_sq = int(consts[1]), int(consts[2]), float(consts[3])
    curve = {1: 0.225, 2: 0.329, 4: 0.457, 8: 0.761, 16: 1.289}  # intervals of 50 steps: largest of four windows, 3 000 steps thermalised
    bound = min(v for k, v in curve.items() if k >= every)
    assert 1e-3 * milli >= 1.15 * 2 * bound, (every, milli, bound)
    assert 0.24 < stale_sq < 0.25  # (of a margin of 1) half the margin, a little less: the filter gives up early, never late


def test_first_build_and_every_kth_rebuild_are_wide(plan):
    _, b = plan(50, 0, 0, 1000)
    assert b[0] == (0, "wide first")
    assert [k for k, _ in b] == list(range(0, 1000, 50))
    assert [k for k, what in b if what.startswith("wide")] == [0, 400, 800]  # kCandEvery = 8 rebuilds per wide build
    _, b = plan(5, 3, 0, 41)
    assert [k for k, what in b if what.startswith("wide")] == [0, 15, 30] and len(b) == 9


@pytest.mark.parametrize("a", [13, 14, 15, 16, 17, 30, 31])
def test_two_calls_schedule_as_one(plan, a):
    """advance(a); advance(b) issues the builds of advance(a + b): a split before, on and behind a wide build, and one
    that starts ``since_build`` steps into an interval."""
    _, whole = plan(5, 3, 0, 46)
    _, split = plan(5, 3, 0, a, 46 - a)
    assert split == whole


def test_a_recovery_is_wide_and_restarts_the_count(plan):
    _, b = plan(5, 3, 0, 60, "r22")
    assert (22, "wide recovery") in b
    after = [(k, w) for k, w in b if k > 22]
    assert [k for k, _ in after] == [27, 32, 37, 42, 47, 52, 57]  # the interval restarts at the recovery too
    assert [w for _, w in after] == ["filter", "filter", "wide", "filter", "filter", "wide", "filter"]


def test_a_load_and_another_margin_start_from_a_wide_build(plan):
    _, b = plan(5, 3, 0, 12, "load", 12)
    assert b == [(0, "wide first"), (5, "filter"), (10, "filter"), (12, "wide first"), (17, "filter"), (22, "filter")]
    _, b = plan(5, 8, 0, 12, "margin=400", 12)
    assert b == [(0, "wide first"), (5, "filter"), (10, "filter"), (15, "wide"), (20, "filter")]
