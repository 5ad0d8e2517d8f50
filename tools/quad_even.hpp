// The archived prototypes (lu_bench, blocked_bench, chol_bench, tri3_bench, quad_square.hpp,
// spkd_blocked.hpp) were written for the even row split, 13 rows in each slot and lanes
// 13..15 idle; the library has since moved to 7/16/16 (spkd_quad.hpp).  This header pins the
// even split for a tool and names its slot height.  Include it before any library header.
#pragma once
#ifdef SPKD_QUAD_BASES
#error "include quad_even.hpp before the library's headers"
#endif
#define SPKD_QUAD_BASES 0, 13, 26
#include "spkd_quad.hpp"

namespace spkd {
constexpr int QL = 13;        // rows per slot
static_assert(quad_rows(0) == QL && quad_rows(1) == QL && quad_rows(2) == QL, "even split");
}  // namespace spkd
