// graph_table.hpp — a training batch's compact image assembled on the device from a resident table of
// per-molecule codes (wdmpnn.h "Resident graph tables", wdmpnn_gather_compact).
//
// A molecule's compact record is position-independent (WdAtomCode holds nothing batch-relative, WdBondPair's
// endpoints are molecule-local), so the atoms / pairs / xn sections of any batch's image are a segmented copy
// of the table's records to the places the host plan (compact.hpp plan_sizes) gave them in `mols`.
//
// One wave per molecule, not a flat grid over records.  Every molecule of a table fits one molecule block
// (<= 64 atoms, <= 128 directed bonds = 64 pairs: the table refuses others), so the 64 lanes of a wave cover
// its atom records in one pass and its pair records in another: one 128-bit load and one 128-bit store per
// record per lane, and the molecule's scope (four words of `mols`, one id, two offsets) is read once per wave
// through wave-uniform addresses.  A flat grid would have every lane bisect the batch's scopes first: about
// log2(B) dependent loads in front of each 16-byte copy, for a kernel that is pure latency at B = 50.  (The
// loops below still step by 64, so a larger record count would be copied whole, not cut.)
//
// Pure copies: every payload bit is preserved.  No atomics, no LDS, plain vector stores, a fixed
// thread-to-record map.  Nothing is clamped (like wdmpnn_join_rows): ids reach the kernel only through an
// index validated on the host.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace wd {

struct GatherCompactArgs {
    const uint4 *t_atoms, *t_pairs;  // the table's records, 16 bytes each
    const float *t_xn;
    const int64_t *t_first;          // [table molecules][2]: first atom record, first pair record
    const int64_t *ids;              // [n_rows] validated table rows
    const int32_t *mols;             // destination image: [n_mols][4]
    uint4 *atoms, *pairs;            // destination image sections
    float *xn;
    int n_mols, n_rows, n_slots, slot0;
};

__global__ __launch_bounds__(256) void gather_compact_kernel(const GatherCompactArgs A) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
    if (m >= A.n_mols) return;
    // batch molecule m = slot (slot0 + m / n_rows) of table row ids[m % n_rows]
    const int64_t id = A.ids[m % A.n_rows] * A.n_slots + A.slot0 + m / A.n_rows;
    const int4 r = *reinterpret_cast<const int4 *>(A.mols + 4 * (size_t)m);  // atom_start, n_atoms, bond_start, n_bonds
    const int64_t a0 = A.t_first[2 * id], p0 = A.t_first[2 * id + 1];
    const uint4 *sa = A.t_atoms + a0;
    uint4 *da = A.atoms + r.x;
    for (int i = lane; i < r.y; i += 64) da[i] = sa[i];
    const uint4 *sp = A.t_pairs + p0;
    uint4 *dp = A.pairs + (r.z - 1) / 2;
    const int np = r.w >> 1;
    for (int i = lane; i < np; i += 64) dp[i] = sp[i];
    if (lane == 0) {
        A.xn[m] = A.t_xn[id];
        if (m == 0) {  // the pad atom row 0 (compact::pad_atom): no columns, last = 0, w = 0
            uint4 pad;
            pad.x = 0xFFFFFFFFu; pad.y = 0xFFFFFFFFu; pad.z = 0u; pad.w = 0u;
            A.atoms[0] = pad;
        }
    }
}

}  // namespace wd
