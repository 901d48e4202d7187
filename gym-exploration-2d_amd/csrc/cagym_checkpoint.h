// cagym_checkpoint.h -- whole-handle checkpoint (include/cagym.h: cagym_checkpoint_sizes / _save / _load).
//
// A checkpoint's device blob is five sections back to back.  The rows of worlds and the rows of pool slots move through
// k_snapshot_copy (cagym_snapshot.h: SNAP_GATHER / SNAP_SCATTER and their slot-indexed twins).  Everything else the handle keeps on
// the device for a streamed run - the stream's words, the episode log, the replay buffer - is a handful of flat arrays of very
// different sizes (4 bytes to capacity * M doubles), and one kernel moves them all: k_checkpoint_flat, driven like k_snapshot_copy
// by a field table that travels BY VALUE in the kernel arguments, every entry {device base pointer, bytes, offset inside the flat
// part of the blob}.  The lanes of the whole grid stride over that flat part in 16-byte chunks; every field starts at a multiple
// of 16 there, so a chunk lies in one field, which the lane finds by a scan of the table (uniform loads, selects).  A chunk moves
// as one 16-byte access where the field's base is 16-byte aligned and the chunk lies inside the field, else as 4-byte words and,
// for the tail of a byte column whose length is no multiple of 4 (the log's flags), single bytes.  Plain vector loads and stores
// only: no LDS, no atomics, no waits.  The host computes every offset and size (cagym_api.hip: ckpt_flat_table), so the kernel reads
// nothing from the blob that could lead it out of bounds.
#pragma once
#include "cagym_device.h"

#define CKPT_MAX_FIELDS 32
#define CKPT_NT 256
#define CKPT_MAX_GRID 1024

struct CkptField {
    unsigned char* base;  // the handle's array; 4-byte aligned at least
    uint64_t bytes;
    uint64_t off;  // inside the flat part of the blob, a multiple of 16, ascending; the first is 0
};

struct CkptTable {
    int n_fields;
    int to_blob;     // 1: handle -> blob (save), 0: blob -> handle (load)
    uint64_t bytes;  // of the flat part: every field rounded up to 16
    CkptField f[CKPT_MAX_FIELDS];
};

__global__ void __launch_bounds__(CKPT_NT) k_checkpoint_flat(CkptTable T, unsigned char* flat) {
    const uint64_t stride = 16ull * CKPT_NT * gridDim.x;
    for (uint64_t c = 16ull * ((uint64_t)blockIdx.x * CKPT_NT + threadIdx.x); c < T.bytes; c += stride) {
        // the field chunk c lies in: the last one that starts at or before it
        unsigned char* base = nullptr;
        uint64_t bytes = 0, off = 0;
        for (int k = 0; k < T.n_fields; k++) {
            const bool hit = T.f[k].off <= c;
            base = hit ? T.f[k].base : base;
            bytes = hit ? T.f[k].bytes : bytes;
            off = hit ? T.f[k].off : off;
        }
        const uint64_t o = c - off;  // < bytes rounded up to 16
        if (o >= bytes) continue;
        const unsigned char* s = T.to_blob ? base + o : flat + c;
        unsigned char* d = T.to_blob ? flat + c : base + o;
        if (o + 16u <= bytes && ((uint32_t)reinterpret_cast<uintptr_t>(base) & 15u) == 0) {
            *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(s);
            continue;
        }
        const uint32_t left = (uint32_t)(bytes - o < 16u ? bytes - o : 16u), nw = left >> 2;
        uint32_t w[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++)
            if (j < nw) w[j] = reinterpret_cast<const uint32_t*>(s)[j];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++)
            if (j < nw) reinterpret_cast<uint32_t*>(d)[j] = w[j];
        for (uint32_t j = 4u * nw; j < left; j++) d[j] = s[j];
    }
}
