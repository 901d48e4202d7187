// cagym_snapshot.h -- per-world state snapshot, restore and fork (include/cagym.h: cagym_snapshot / cagym_restore / cagym_fork).
//
// One copy kernel beside the step kernels, driven by a field table that travels BY VALUE in the kernel arguments: every entry is
// {device base pointer, bytes per row, offset inside a blob row}.  One 256-lane workgroup moves one row (one world, or one
// scenario slot of the pool).  Its lanes stride over the ROW - the blob row, or the same packing of the fields when no blob is
// involved - in 16-byte chunks; every field starts at a multiple of 16 there, so a chunk lies in one field, which the lane
// finds by a scan of the table (uniform loads, selects).  All loads of a row are therefore in flight together: a first version
// that walked the fields one after the other, five active lanes at a time for an 80-byte field, took ~30 dependent round trips
// per row.  A chunk moves as one 16-byte access where the field's row size and base are multiples of 16 (M = 4, 10, 20: every
// fp64 field), else as up to four 4-byte words (every field of the handle is made of 4- or 8-byte elements).  Plain vector
// loads and stores only: no LDS, no atomics, no waits.
//
// The four directions (SnapTable::mode):
//   SNAP_GATHER   SoA row of world ids[r] (null: r)              -> blob row r, whose header takes the origin world id
//   SNAP_SCATTER  blob row ids[r] (null: r)                      -> SoA row of the origin world its header names
//   SNAP_FORK     SoA row of world ids[r]                        -> SoA row of world ids2[r]
//   SNAP_POOL     pool row of the scenario slot of world ids[r]  -> pool row of the scenario slot of world ids2[r]
//   SNAP_SLOT_GATHER   pool row of slot r                        -> blob row r, whose header takes the slot   (cagym_checkpoint_save)
//   SNAP_SLOT_SCATTER  blob row r                                -> pool row of the slot its header names      (cagym_checkpoint_load)
// Every id read from a caller's list (and the origin id read from a blob header) is checked against [0, N) - a slot against
// [0, S) -: a workgroup that finds one outside returns before it touches anything else, so a wrong list cannot fault the device.
//
// A world's scenario slot is computed, not stored: (world + episode[world] * N) % S, as every kernel derives it
// (cagym_sensors.h, cagym_ig.h).  SNAP_POOL reads `episode` of both worlds; cagym_fork leaves dst's episode as it is, so the two
// fork launches commute.
#pragma once
#include "cagym_device.h"

#define SNAP_MAX_FIELDS 44
#define SNAP_NT 256
#define SNAP_HEADER_BYTES 16 /* {origin world id, CAGYM_SNAP_MAGIC, 0, 0} */

enum { SNAP_GATHER = 0, SNAP_SCATTER = 1, SNAP_FORK = 2, SNAP_POOL = 3, SNAP_SLOT_GATHER = 4, SNAP_SLOT_SCATTER = 5 };

struct SnapField {
    unsigned char* base;  // row r of the field starts at base + r * bytes
    uint32_t bytes;       // per row; a multiple of 4
    uint32_t off;         // inside a blob row, a multiple of 16, ascending; SNAP_FORK / SNAP_POOL pack their fields the same way
};

struct SnapTable {
    int mode, n_fields;
    int N, S;                // bounds of the ids; S and `episode` serve SNAP_POOL's slot arithmetic
    const int32_t* episode;  // [N]
    uint64_t row_bytes;      // of a blob row (of the packed fields): header + every field rounded up to 16
    SnapField f[SNAP_MAX_FIELDS];
};

__global__ void __launch_bounds__(SNAP_NT) k_snapshot_copy(SnapTable T, const int32_t* __restrict__ ids, const int32_t* __restrict__ ids2,
                                                           unsigned char* blob) {
    const int r = blockIdx.x, tid = threadIdx.x;
    const bool slots = T.mode >= SNAP_SLOT_GATHER;  // rows of the pool: ids and headers are slots, bounded by S
    const bool gather = T.mode == SNAP_GATHER || T.mode == SNAP_SLOT_GATHER, scatter = T.mode == SNAP_SCATTER || T.mode == SNAP_SLOT_SCATTER;
    const long long rows = slots ? T.S : T.N;
    const uint32_t magic = slots ? CAGYM_CKPT_ROW_MAGIC : CAGYM_SNAP_MAGIC;
    const long long a = ids ? ids[r] : r;
    if (a < 0 || a >= rows) return;  // a world id or a slot, or a blob row id (a blob holds at most N rows, of slots S)
    long long src_row = a, dst_row = a;
    unsigned char* brow = nullptr;
    if (gather) {
        brow = blob + (size_t)r * T.row_bytes;
        if (tid == 0) *reinterpret_cast<uint4*>(brow) = make_uint4((uint32_t)a, magic, 0u, 0u);
    } else if (scatter) {
        brow = blob + (size_t)a * T.row_bytes;
        const uint4 h = *reinterpret_cast<const uint4*>(brow);
        dst_row = (int32_t)h.x;
        if (h.y != magic || dst_row < 0 || dst_row >= rows) return;  // not a row cagym_snapshot / cagym_checkpoint_save wrote
    } else {
        const long long b = ids2[r];
        if (b < 0 || b >= T.N) return;
        dst_row = b;
        if (T.mode == SNAP_POOL) {
            src_row = (a + (long long)T.episode[a] * T.N) % T.S;
            dst_row = (b + (long long)T.episode[b] * T.N) % T.S;
            if (src_row < 0 || dst_row < 0) return;  // a negative episode index: no kernel writes one
        }
        if (src_row == dst_row) return;
    }
    for (uint32_t c = SNAP_HEADER_BYTES + 16u * tid; c < (uint32_t)T.row_bytes; c += 16u * SNAP_NT) {
        // the field chunk c lies in: the last one that starts at or before it (offsets ascend; the first is SNAP_HEADER_BYTES)
        unsigned char* base = nullptr;
        uint32_t bytes = 0, off = 0;
        for (int k = 0; k < T.n_fields; k++) {
            const bool hit = T.f[k].off <= c;
            base = hit ? T.f[k].base : base;
            bytes = hit ? T.f[k].bytes : bytes;
            off = hit ? T.f[k].off : off;
        }
        const uint32_t o = c - off;  // < bytes rounded up to 16
        const unsigned char* s = scatter ? brow + c : base + (size_t)src_row * bytes + o;
        unsigned char* d = gather ? brow + c : base + (size_t)dst_row * bytes + o;
        if (((bytes | (uint32_t)reinterpret_cast<uintptr_t>(base)) & 15u) == 0) {
            *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(s);
        } else {
            uint32_t w[4];
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (o + 4u * j < bytes) w[j] = reinterpret_cast<const uint32_t*>(s)[j];
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (o + 4u * j < bytes) reinterpret_cast<uint32_t*>(d)[j] = w[j];
        }
    }
}
