// table_profile.h -- what the table profile's two entry points share (csrc/table_profile.hip: gsx_table_profile_dev,
// csrc/host_rows.hip: gsx_table_profile_host): the argument rules and the 48 byte offsets both walk.
#pragma once
#include "gsx_common.h"

namespace gsx {

constexpr int PROFILE_FIELDS = 48;       // x y z | f_rest_0..44
constexpr int PROFILE_MAX_ROW_BYTES = 512;   // row_tile.h: SPZ_MAX_ROW_BYTES

struct ProfileOffsets {
    int off[PROFILE_FIELDS];             // byte offset inside a row, -1 = absent
};

// gsx_profile_layout -> ProfileOffsets: n >= 1, the row size in range, every present field inside a row
static int profile_layout_check(const gsx_profile_layout *l, int64_t n, ProfileOffsets *out, const char *who)
{
    if (!l) GSX_FAIL("%s: null layout", who);
    if (n < 1 || n >= (1LL << 32)) GSX_FAIL("%s: 1 <= n < 2^32", who);
    if (l->row_bytes < 1 || l->row_bytes > PROFILE_MAX_ROW_BYTES)
        GSX_FAIL("%s: rows of %lld bytes (1 ... %d are supported)", who, (long long)l->row_bytes, PROFILE_MAX_ROW_BYTES);
    for (int f = 0; f < PROFILE_FIELDS; ++f) {
        const int o = f < 3 ? l->xyz_offset[f] : l->rest_offset[f - 3];
        if (o >= 0 && o + 4 > l->row_bytes)
            GSX_FAIL("%s: field %d at byte offset %d of a %lld-byte row", who, f, o, (long long)l->row_bytes);
        out->off[f] = o < 0 ? -1 : o;
    }
    return 0;
}

}  // namespace gsx
