// Stand-alone check of the parts of csrc/gba_solve.h that place memory and deal out indices, built with
// -fsanitize=address,undefined by tests/test_gba_edge_host.py (no HIP, no GPU):
//  * gba::layout measured and placed for 0 / 1 / 65 / 1024 free cameras: every piece inside the block, 256-byte
//    aligned, disjoint from every other, and the size a function of the actual counts (S takes 6 F x (6 F + 1) doubles,
//    nothing for F = 0);
//  * the tile schedule for every n in 0 .. 4 T + 7: in each step of each tile column, every entry of the lower triangle
//    in that column and of the extra row is covered exactly once, and nothing outside is;
//  * the tiled solve on a small system, so that the sanitizers see every index it forms.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "gba_solve.h"

using namespace msf;

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
      return 1;                                                   \
    }                                                             \
  } while (0)

static int check_layout(size_t cams, size_t points, size_t edges, int nf, size_t* bytes) {
  Carver measure;
  gba::layout(measure, cams, points, edges, nf);
  std::vector<uint8_t> block(measure.off + 512);
  uint8_t* base = block.data();
  base += (256 - (uintptr_t)base % 256) % 256;
  Carver place{base};
  const gba::Scratch s = gba::layout(place, cams, points, edges, nf);
  CHECK(place.off == measure.off);
  const size_t f = (size_t)nf, n = 6 * f;
  const ba::Scratch& w = s.w;
  const std::pair<const void*, size_t> pieces[] = {
      {s.rec, sizeof(gba::Record)},   {w.cam, cams * sizeof(ba::Estimate)}, {w.cam_trial, cams * sizeof(ba::Estimate)},
      {w.pt, points * 24},            {w.pt_trial, points * 24},            {w.free_of, cams * 4},
      {w.free_cam, cams * 4},         {w.cam_start, cams * 4},              {w.cam_end, cams * 4},
      {w.cam_edges, edges * 4},       {w.cam_active, cams * 4},             {w.pt_start, points * 4},
      {w.pt_end, points * 4},         {w.pt_active, points * 4},            {w.word, 4},
      {w.active, edges},              {w.chi2_0, edges * 8},                {w.lin, edges * ba::kLin * 8},
      {w.W, edges * 18 * 8},          {w.Hpp, points * 48},                 {w.bp, points * 24},
      {w.inv, points * 48},           {w.dxp, points * 24},                 {w.redp, points * 8},
      {w.redq, points * 8},           {w.redc, cams * 8},                   {w.Hcc, f * 27 * 8},
      {w.S, n * (n + 1) * 8},         {w.diag, n * 8},                      {w.x, n * 8}};
  size_t sum = 0;
  for (const auto& a : pieces) {
    if (!a.second) continue;
    const uint8_t* p = (const uint8_t*)a.first;
    CHECK((uintptr_t)p % 256 == 0);
    CHECK(p >= base && p + a.second <= base + measure.off);
    for (const auto& b : pieces) {
      const uint8_t* q = (const uint8_t*)b.first;
      if (&a == &b || !b.second) continue;
      CHECK(p + a.second <= q || q + b.second <= p);
    }
    sum += (a.second + 255) & ~(size_t)255;
  }
  CHECK(sum == measure.off);   // nothing but the pieces: the size follows from the counts
  CHECK(w.max_free == nf);
  *bytes = measure.off;
  return 0;
}

static int check_schedule(int n) {
  const int T = gba::kTile;
  CHECK(gba::panels(n) == (n + T - 1) / T);
  std::vector<int> seen((size_t)(n + 1) * (n > 0 ? n : 1));
  const auto clear = [&]() { std::fill(seen.begin(), seen.end(), 0); };
  const auto mark = [&](int i, int j) {
    if (i < j || i > n || j < 0 || j >= n) return false;
    seen[(size_t)j * (n + 1) + i]++;
    return true;
  };
  const auto covered = [&](int J) {   // every (i, j), j in panel J, j <= i <= n, exactly once; nothing else
    for (int j = 0; j < n; j++)
      for (int i = 0; i <= n; i++) {
        const bool in = j >= gba::col0(J) && j < gba::col1(n, J) && i >= j;
        if (seen[(size_t)j * (n + 1) + i] != (in ? 1 : 0)) return false;
      }
    return true;
  };
  int last_col = 0;
  for (int J = 0; J < gba::panels(n); J++) {
    CHECK(gba::col0(J) == last_col && gba::col1(n, J) > gba::col0(J) && gba::col1(n, J) <= n);
    last_col = gba::col1(n, J);
    // step 1: tiles I >= J
    clear();
    for (int I = J; I < gba::row_tiles(n); I++) {
      CHECK(gba::row0(I) < gba::row1(n, I) && gba::row1(n, I) - gba::row0(I) <= T);
      for (int j = gba::col0(J); j < gba::col1(n, J); j++)
        for (int i = gba::row0(I) > j ? gba::row0(I) : j; i < gba::row1(n, I); i++) CHECK(mark(i, j));
    }
    CHECK(covered(J));
    // steps 2 and 3: the diagonal tile, then the tiles below
    clear();
    for (int j = gba::col0(J); j < gba::col1(n, J); j++)
      for (int i = j; i < gba::row1(n, J); i++) CHECK(mark(i, j));
    for (int I = J + 1; I < gba::row_tiles(n); I++)
      for (int i = gba::row0(I); i < gba::row1(n, I); i++)
        for (int j = gba::col0(J); j < gba::col1(n, J); j++) CHECK(mark(i, j));
    CHECK(covered(J));
  }
  CHECK(last_col == n);
  CHECK(gba::row1(n, gba::row_tiles(n) - 1) == n + 1);
  // the back substitution's blocks are the tile columns, last first; the rows above a block are 0 .. b0 - 1
  return 0;
}

static int check_solve(int n) {
  std::vector<double> S((size_t)n * (n + 1)), R, diag(n), x(n), diag2(n), x2(n);
  for (int j = 0; j < n; j++) {
    for (int i = j; i < n; i++) S[(size_t)j * (n + 1) + i] = i == j ? n + 1.0 : 1.0 / (1 + i - j);
    S[(size_t)j * (n + 1) + n] = j % 7 - 3.0;
  }
  R = S;
  CHECK(gba::cholesky(S.data(), n, diag.data()) == -1);
  gba::back_substitute(S.data(), n, diag.data(), x.data());
  CHECK(ba::cholesky(ba::Serial(), R.data(), n, diag2.data()));
  ba::back_substitute(ba::Serial(), R.data(), n, diag2.data(), x2.data());
  for (int j = 0; j < n; j++) CHECK(x[j] == x2[j] && diag[j] == diag2[j]);
  return 0;
}

int main() {
  size_t b0 = 0, b1 = 0, b65 = 0, b1024 = 0, other = 0;
  if (check_layout(3, 7, 11, 0, &b0) || check_layout(3, 7, 11, 1, &b1) || check_layout(70, 300, 1200, 65, &b65) ||
      check_layout(1030, 5000, 20000, 1024, &b1024) || check_layout(1030, 5000, 20000, 65, &other))
    return 1;
  CHECK(b1 > b0 && b1 - b0 == 256 + ((6 * 7 * 8 + 255) & ~255) + 256 + 256);   // Hcc, S, diag, x of one camera
  CHECK(b1024 - other > (size_t)6144 * 6145 * 8 - (size_t)390 * 391 * 8);      // sized by the free cameras, not by the cap
  CHECK(b65 < (size_t)8 << 20);
  for (int n = 0; n <= 4 * gba::kTile + 7; n++)
    if (check_schedule(n)) return 1;
  for (int n : {1, 63, 64, 65, 130})
    if (check_solve(n)) return 1;
  std::printf("gba edge checks passed\n");
  return 0;
}
