// cagym_layout.h -- host only: how the C ABI (cagym_api.hip) lays out a block of device arrays that share one allocation.  Nothing
// here includes HIP: tests/test_layout_host.py compiles tests/layout_check.cpp against it with the host compiler's sanitizers.
// A block is written ONCE, as a function that presents every member with its element count to a visitor:
//     template <class V> constexpr void replay_table_members(ReplayDev& R, size_t S, V& v) { v(R.words, RPW_WORDS); v(R.buf_gen, 1); ... }
// and the visitors turn that listing into the allocation's size (LayoutBytes), the members' pointers handed out from its base
// (LayoutCarve), the {base, bytes, offset} entries of a checkpoint table for the members a checkpoint carries (LayoutCkpt; applied to
// an empty struct: the sizes and offsets before anything is allocated) and their number at compile time (LayoutCount).
// Every member starts at a multiple of 16 bytes, in device memory and in the blob alike, so an 8-byte member may follow a 4-byte
// one and the listing's order is free to be the blob's order.  A member no checkpoint carries is presented with LAYOUT_SCRATCH.
#pragma once
#include <cstddef>
#include <cstdint>

constexpr size_t layout_round16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }
constexpr bool LAYOUT_SCRATCH = false;  // v(member, count, LAYOUT_SCRATCH)

struct LayoutBytes {
    size_t bytes = 0;
    template <typename T>
    constexpr void operator()(T*&, size_t count, bool = true) { bytes += layout_round16(sizeof(T) * count); }
};
struct LayoutCarve {
    unsigned char* base;
    size_t off = 0;
    template <typename T>
    void operator()(T*& member, size_t count, bool = true) {
        member = reinterpret_cast<T*>(base + off);
        off += layout_round16(sizeof(T) * count);
    }
};
// Table: {int n_fields; Field f[];}, Field: {unsigned char* base; uint64_t bytes, off;}; `off` runs on from block to block of a blob
template <typename Table>
struct LayoutCkpt {
    Table& table;
    uint64_t& off;
    template <typename T>
    void operator()(T*& member, size_t count, bool in_checkpoint = true) {
        if (!in_checkpoint) return;
        table.f[table.n_fields++] = {reinterpret_cast<unsigned char*>(member), sizeof(T) * (uint64_t)count, off};
        off += layout_round16(sizeof(T) * count);
    }
};
struct LayoutCount {
    int n = 0;
    template <typename T>
    constexpr void operator()(T*&, size_t, bool in_checkpoint = true) { n += in_checkpoint ? 1 : 0; }
};
