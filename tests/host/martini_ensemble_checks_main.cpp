// Stand-alone host program for mythos_amd/csrc/martini_ensemble_checks.h and the chunking of martini_exchange_checks.h, built with -fsanitize=address,undefined by
// tests/test_martini_ensemble_cpu.py: the refusals of the ensemble's creation and load on arrays of exactly the length
// they are said to have, and the chunking of an advance under a barostat over R records per row, written into buffers of
// exactly the size the C ABI documents.  Exit code 0 and "ok" on success.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "martini_ensemble_checks.h"
#include "martini_exchange_checks.h"

namespace mythos {
static std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }
}  // namespace mythos

using namespace mythos;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "line %d: %s (last error: %s)\n", __LINE__, #cond, g_error.c_str()); \
      return 1;                                                            \
    }                                                                      \
  } while (0)

static bool has(const char* part) { return g_error.find(part) != std::string::npos; }

int main() {
  // ---- refusals
  {
    std::vector<double> kT{2.27, 2.5, 2.66};
    std::vector<double> boxes{6.4, 6.5, 10.0, 6.4, 6.5, 10.0, 6.4, 6.5, 10.0};
    CHECK(mm_ensemble_check(1280, 3, kT.data(), 1.1, 0.25, boxes.data(), "t") == 0);
    CHECK(mm_ensemble_check(1280, 3, kT.data(), 1.1, 0.25, nullptr, "t") == 0);
    CHECK(mm_ensemble_check(1280, 0, kT.data(), 1.1, 0.25, nullptr, "t") == -1 && has("n_rep >= 1"));
    CHECK(mm_ensemble_check(0, 3, kT.data(), 1.1, 0.25, nullptr, "t") == -1 && has("at least one bead"));
    CHECK(mm_ensemble_check(1280, 3, nullptr, 1.1, 0.25, nullptr, "t") == -1);
    kT[2] = 0.0;
    CHECK(mm_ensemble_check(1280, 3, kT.data(), 1.1, 0.25, nullptr, "t") == -1 && has("kT of replica 2"));
    kT[2] = std::nan("");
    CHECK(mm_ensemble_check(1280, 3, kT.data(), 1.1, 0.25, nullptr, "t") == -1 && has("kT of replica 2"));
    kT[2] = 2.66;
    boxes[5] = 2.6;
    CHECK(mm_ensemble_check(1280, 3, kT.data(), 1.1, 0.25, boxes.data(), "t") == -1 && has("replica 1: the box is smaller"));
    boxes[5] = -1.0;
    CHECK(mm_ensemble_check(1280, 3, kT.data(), 1.1, 0.25, boxes.data(), "t") == -1 && has("replica 1: invalid argument"));
    std::vector<double> many(4, 1.0);
    CHECK(mm_ensemble_check(1 << 21, 4, many.data(), 1.1, 0.25, nullptr, "t") == -1 && has("rows the neighbour store indexes"));
    CHECK(mm_ensemble_check((INT_MAX / kMmStride0) / 4, 4, many.data(), 1.1, 0.25, nullptr, "t") == 0);
    const double edge[3] = {2.7, 3.0, 3.4};  // exactly 2 (1.1 + 0.25)
    CHECK(mm_box_fits(edge, 1.1 + 0.25, "t") == 0);
    CHECK(mm_box_fits(nullptr, 1.35, "t") == -1);
  }
  // ---- chunking: every combination walks the call as mm_advance_chunked does under a barostat alone and writes its rows
  long chunks = 0;
  for (int copies : {1, 3, 16})
    for (int every : {1, 2, 3, 10, 12})
      for (int save_every : {0, 1, 3, 4, 10})
        for (int n_steps : {1, 5, 12, 24, 37})
          for (int64_t step0 : {0, 1, 7, 12, 1000003}) {
            const int n_rows = save_every > 0 ? n_steps / save_every : 0;
            const size_t width = 5;
            std::vector<double> trace((size_t)n_rows * copies * width, -1.0), boxes((size_t)n_rows * copies * 3, -1.0);
            int64_t step = step0;
            int done = 0, rows = 0, events = 0;
            while (done < n_steps) {
              const MmEventChunk c = mm_event_chunk(step, every, 0, done, n_steps, save_every);
              CHECK(c.len >= 1 && done + c.len <= n_steps);
              step += c.len, done += c.len, ++chunks;
              CHECK(c.couple == (step % every == 0) && !c.exchange);
              CHECK(c.save == (save_every > 0 && done % save_every == 0));
              CHECK(c.last == (done == n_steps));
              if (c.save) {
                CHECK(rows < n_rows);
                double* t = trace.data() + mm_row_offset(rows, copies, width);
                double* b = boxes.data() + mm_row_offset(rows, copies, 3);
                for (int r = 0; r < copies; ++r) {
                  for (size_t k = 0; k < width; ++k) t[r * width + k] = double(done);
                  for (int d = 0; d < 3; ++d) b[3 * r + d] = double(done);
                }
                ++rows;
              }
              if (c.couple) ++events;
            }
            CHECK(done == n_steps && rows == n_rows);
            CHECK(events == (int)((step0 + n_steps) / every - step0 / every));
            for (size_t k = 0; k < trace.size(); ++k) CHECK(trace[k] == double((k / (copies * width) + 1) * save_every));
            for (double v : boxes) CHECK(v > 0);
          }
  std::printf("ok (%ld chunks)\n", chunks);
  return 0;
}
