// Stand-alone CPU driver of bluesky_amd/csrc/bsa_route_math.h (the host +
// device inline part of the route edits) over the edge shapes
// of tests/test_gpu_route_edit.py: the stable grouping, the per-aircraft check
// and row counts, the iactwp rules and the backward VNAV pass in chunks of 64.
// Meant for a sanitizer build on the CPU:
//   c++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined \
//       -I include tools/route_math_check.cpp -o route_math_check && ./route_math_check
#include <cstdio>
#include <cstdlib>

#include "../bluesky_amd/csrc/bsa_route_math.h"

using namespace bsa::route;

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);  \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

static bsa_route_edit_rec rec(int ac, int op, int pos, int type = 0, double lat = 52., double lon = 4.) {
  return bsa_route_edit_rec{ac, op, pos, 1, type, 0, lat, lon, -999., -999.};
}

// the VNAV pass over a whole route at once and in chunks of 64 from the end: the same bits
static void vnav_case(int n, unsigned seed) {
  std::vector<double> alt((size_t)n), dist((size_t)n), t1((size_t)n), x1((size_t)n), t2((size_t)n), x2((size_t)n);
  std::vector<int> type((size_t)n);
  for (int i = 0; i < n; ++i) {
    seed = seed * 1664525u + 1013904223u;
    alt[(size_t)i] = (seed >> 28) < 3 ? 1000. * (seed >> 24 & 15) : -999.;
    type[(size_t)i] = (i == n - 1 && (seed & 1)) ? kTypeDest : 0;
    dist[(size_t)i] = 1. + (seed >> 8 & 1023) / 97.;
  }
  Vnav a;
  vnav_pass(a, 0, n, n, alt.data(), type.data(), dist.data(), t1.data(), x1.data());
  Vnav b;
  for (int i1 = n; i1 > 0; i1 -= 64) {
    const int i0 = i1 > 64 ? i1 - 64 : 0;
    vnav_pass(b, i0, i1, n, alt.data() + i0, type.data() + i0, dist.data() + i0, t2.data() + i0, x2.data() + i0);
  }
  for (int i = 0; i < n; ++i) CHECK(t1[(size_t)i] == t2[(size_t)i] && x1[(size_t)i] == x2[(size_t)i]);
  // by hand: the running sum in the reference's order of additions
  double toalt = -999., xtoalt = 0.;
  for (int i = n - 1; i >= 0; --i) {
    if (type[(size_t)i] == kTypeDest) toalt = 0., xtoalt = 0.;
    else if (alt[(size_t)i] >= 0) toalt = alt[(size_t)i], xtoalt = 0.;
    else if (i != n - 1) xtoalt += dist[(size_t)i] * 1852.;
    else xtoalt = 0.;
    CHECK(t1[(size_t)i] == toalt && x1[(size_t)i] == xtoalt);
  }
}

int main() {
  // ---- grouping: stable, records of one aircraft not adjacent, an empty batch
  {
    const bsa_route_edit_rec b[] = {rec(7, 0, 0), rec(2, 2, 1), rec(7, 2, 0), rec(0, 3, 2), rec(2, 0, 0), rec(7, 0, 1)};
    std::vector<int32_t> order, gs;
    CHECK(group(6, b, order, gs) == 3);
    const int32_t eo[] = {3, 1, 4, 0, 2, 5}, eg[] = {0, 1, 3, 6};
    for (int q = 0; q < 6; ++q) CHECK(order[(size_t)q] == eo[q]);
    for (int q = 0; q < 4; ++q) CHECK(gs[(size_t)q] == eg[q]);
    CHECK(group(0, nullptr, order, gs) == 0 && gs.size() == 1 && order.empty());
    CHECK(group(1, b, order, gs) == 1 && gs[1] == 1);
  }
  // ---- counts and refusals against the route the earlier records left
  {
    const bsa_route_edit_rec b[] = {rec(0, BSA_ROUTE_INSERT, 64), rec(0, BSA_ROUTE_INSERT, 65), rec(0, BSA_ROUTE_DELETE, 0),
                                    rec(0, BSA_ROUTE_DELETE, 64), rec(0, BSA_ROUTE_DIRECT, 63)};
    const int32_t ord[] = {0, 1, 2, 3, 4};
    int nf = 0, nmax = 0, bad = -1;
    CHECK(plan(b, ord, 5, 64, &nf, &nmax, &bad) == BSA_ROUTE_OK && nf == 64 && nmax == 66);
    CHECK(plan(b, ord, 5, 63, &nf, &nmax, &bad) == BSA_ROUTE_ERR_POS && bad == 0);
    CHECK(plan(b, ord + 4, 1, 63, &nf, &nmax, &bad) == BSA_ROUTE_ERR_POS);
    CHECK(plan(b, ord, 0, 5, &nf, &nmax, &bad) == BSA_ROUTE_OK && nf == 5 && nmax == 5);
    const bsa_route_edit_rec first = rec(0, BSA_ROUTE_INSERT, 0), only[] = {first, rec(0, BSA_ROUTE_DELETE, 0)};
    CHECK(plan(only, ord, 2, 0, &nf, &nmax, &bad) == BSA_ROUTE_OK && nf == 0 && nmax == 1);
    CHECK(check(rec(0, BSA_ROUTE_DELETE, 0), 0) == BSA_ROUTE_ERR_POS);
    CHECK(check(rec(0, BSA_ROUTE_INSERT, 0, kTypeRunway), 3) == BSA_ROUTE_ERR_WPTYPE);
    CHECK(check(rec(0, BSA_ROUTE_OVERWRITE, 0, kTypeCalc), 3) == BSA_ROUTE_ERR_WPTYPE);
    CHECK(check(rec(0, BSA_ROUTE_INSERT, 0, 0, NAN, 4.), 3) == BSA_ROUTE_ERR_NONFINITE);
    CHECK(check(rec(0, BSA_ROUTE_INSERT, 0, 0, 52., -INFINITY), 3) == BSA_ROUTE_ERR_NONFINITE);
    CHECK(check(rec(0, BSA_ROUTE_OVERWRITE, 3), 3) == BSA_ROUTE_ERR_POS);
    CHECK(check(rec(0, BSA_ROUTE_INSERT, -1), 3) == BSA_ROUTE_ERR_POS);
    CHECK(check(rec(0, 4, 0), 3) == BSA_ROUTE_ERR_OP && check(rec(0, -1, 0), 3) == BSA_ROUTE_ERR_OP);
    CHECK(check(rec(0, BSA_ROUTE_DELETE, 0, kTypeRunway, NAN, NAN), 1) == BSA_ROUTE_OK);  // a delete carries no waypoint
  }
  // ---- iactwp (route.py:578-579, 834-837)
  CHECK(iactwp_after(BSA_ROUTE_INSERT, 2, 1, 2, 5) == 3 && iactwp_after(BSA_ROUTE_INSERT, 2, 1, 1, 5) == 1);
  CHECK(iactwp_after(BSA_ROUTE_INSERT, 2, 0, 3, 5) == 3 && iactwp_after(BSA_ROUTE_INSERT, 0, 1, -1, 1) == -1);
  CHECK(iactwp_after(BSA_ROUTE_DELETE, 1, 0, 3, 3) == 2 && iactwp_after(BSA_ROUTE_DELETE, 1, 0, 1, 3) == 1);
  CHECK(iactwp_after(BSA_ROUTE_DELETE, 3, 0, 3, 3) == 2 && iactwp_after(BSA_ROUTE_DELETE, 0, 0, 0, 0) == -1);
  CHECK(iactwp_after(BSA_ROUTE_DELETE, 0, 0, 1, 1) == 0 && iactwp_after(BSA_ROUTE_DELETE, 0, 0, -1, 2) == -1);
  CHECK(iactwp_after(BSA_ROUTE_OVERWRITE, 0, 1, 2, 4) == 2 && iactwp_after(BSA_ROUTE_DIRECT, 0, 1, 2, 4) == 2);
  // ---- the position wrap (Python's float %)
  CHECK(wrap_lat(52.) == 52. && wrap_lon(-190.) == 170. && wrap_lon(180.) == -180. && wrap_lat(-90.) == -90.);
  // ---- the VNAV pass: 1, 63, 64, 65, 66, 128, 130 waypoints
  for (int n : {1, 2, 63, 64, 65, 66, 128, 129, 130, 200}) vnav_case(n, 12345u + (unsigned)n);
  Vnav v;
  vnav_pass(v, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr);   // an empty route touches nothing
  std::printf("route_math_check ok\n");
  return 0;
}
