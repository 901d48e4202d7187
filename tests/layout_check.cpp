// The block layout visitors of csrc/cagym_layout.h on the host (tests/test_layout_host.py compiles this with the sanitizers).
// Dummy blocks of an 8-byte, a 4-byte and a 1-byte member plus one LAYOUT_SCRATCH member, presented in every order with every
// combination of the counts 0, 1, 3 and 1000; the allocation is exactly LayoutBytes long, so a pointer handed out past it is the
// address sanitizer's to find when the member is written.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "cagym_layout.h"

struct Dummy {
    uint64_t* wide;
    uint32_t* word;
    uint8_t* byte;
    uint32_t* scratch;
};
struct Field {
    unsigned char* base;
    uint64_t bytes, off;
};
struct Table {
    int n_fields;
    Field f[8];
};

// member k of the listing is order[k]: 0 wide, 1 word, 2 byte, 3 scratch
template <class V>
constexpr void dummy_members(Dummy& D, const int* order, const size_t* count, V& v) {
    for (int k = 0; k < 4; k++) {
        if (order[k] == 0) v(D.wide, count[0]);
        if (order[k] == 1) v(D.word, count[1]);
        if (order[k] == 2) v(D.byte, count[2]);
        if (order[k] == 3) v(D.scratch, count[3], LAYOUT_SCRATCH);
    }
}
constexpr int dummy_checkpointed() {
    const int order[4] = {3, 2, 1, 0};
    const size_t count[4] = {1, 1, 1, 1};
    Dummy D{};
    LayoutCount n;
    dummy_members(D, order, count, n);
    return n.n;
}
static_assert(dummy_checkpointed() == 3, "LayoutCount counts the members a checkpoint carries");
static_assert(layout_round16(0) == 0 && layout_round16(1) == 16 && layout_round16(16) == 16 && layout_round16(17) == 32 && layout_round16(14) == 16,
              "the next multiple of 16");

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            printf("layout_check FAILED line %d: %s\n", __LINE__, #cond); \
            return 1;                                                     \
        }                                                                 \
    } while (0)

static int check_case(const int* order, const size_t* count) {
    static const size_t elem[4] = {8, 4, 1, 4};
    Dummy D{};
    LayoutBytes size;
    dummy_members(D, order, count, size);
    CHECK(size.bytes % 16 == 0);
    unsigned char* base = static_cast<unsigned char*>(aligned_alloc(16, std::max<size_t>(size.bytes, 16)));
    CHECK(base && (reinterpret_cast<uintptr_t>(base) & 15) == 0);
    LayoutCarve carve{base};
    dummy_members(D, order, count, carve);
    unsigned char* const ptr[4] = {reinterpret_cast<unsigned char*>(D.wide), reinterpret_cast<unsigned char*>(D.word), D.byte,
                                   reinterpret_cast<unsigned char*>(D.scratch)};
    // the byte sum is the last member's end rounded up to 16; every pointer is 16-aligned and inside the block (an empty member has
    // no byte to be inside with: it may sit at the block's end); no two members overlap
    const int last = order[3];
    CHECK((size_t)(ptr[last] - base) + layout_round16(elem[last] * count[last]) == size.bytes && carve.off == size.bytes);
    for (int a = 0; a < 4; a++) {
        const size_t lo = (size_t)(ptr[a] - base), n = elem[a] * count[a];
        CHECK(ptr[a] >= base && (lo & 15) == 0 && lo + n <= size.bytes && (n == 0 || lo < size.bytes));
        for (int b = 0; b < a; b++) {
            const size_t lo2 = (size_t)(ptr[b] - base), n2 = elem[b] * count[b];
            CHECK(n == 0 || n2 == 0 || lo + n <= lo2 || lo2 + n2 <= lo);
        }
    }
    // every element can be written and read back (all written first: an overlap would show as another member's pattern)
    for (size_t i = 0; i < count[0]; i++) D.wide[i] = 0x1111111111111111ull * 1 + i;
    for (size_t i = 0; i < count[1]; i++) D.word[i] = 0x22220000u + (uint32_t)i;
    for (size_t i = 0; i < count[2]; i++) D.byte[i] = (uint8_t)(0x33 + i);
    for (size_t i = 0; i < count[3]; i++) D.scratch[i] = 0x44440000u + (uint32_t)i;
    for (size_t i = 0; i < count[0]; i++) CHECK(D.wide[i] == 0x1111111111111111ull * 1 + i);
    for (size_t i = 0; i < count[1]; i++) CHECK(D.word[i] == 0x22220000u + (uint32_t)i);
    for (size_t i = 0; i < count[2]; i++) CHECK(D.byte[i] == (uint8_t)(0x33 + i));
    for (size_t i = 0; i < count[3]; i++) CHECK(D.scratch[i] == 0x44440000u + (uint32_t)i);
    // the checkpoint entries: the three flagged members in listing order, packed from the running offset at multiples of 16
    Table T{};
    uint64_t off = 32;  // (a section that does not open the blob)
    LayoutCkpt<Table> ckpt{T, off};
    dummy_members(D, order, count, ckpt);
    CHECK(T.n_fields == 3);
    uint64_t want_off = 32;
    int k = 0;
    for (int j = 0; j < 4; j++) {
        const int a = order[j];
        if (a == 3) continue;
        CHECK(T.f[k].base == ptr[a] && T.f[k].bytes == elem[a] * count[a] && T.f[k].off == want_off && (T.f[k].off & 15) == 0);
        CHECK(k == 0 || T.f[k].off >= T.f[k - 1].off + T.f[k - 1].bytes);
        want_off += layout_round16(elem[a] * count[a]);
        k++;
    }
    CHECK(off == want_off);
    // the sizes-only pass, on an empty struct: the same entries with null bases
    Dummy E{};
    Table S{};
    uint64_t off2 = 32;
    LayoutCkpt<Table> sizes{S, off2};
    dummy_members(E, order, count, sizes);
    CHECK(S.n_fields == 3 && off2 == off);
    for (k = 0; k < 3; k++) CHECK(S.f[k].base == nullptr && S.f[k].bytes == T.f[k].bytes && S.f[k].off == T.f[k].off);
    free(base);
    return 0;
}

int main() {
    static const size_t counts[4] = {0, 1, 3, 1000};
    int order[4] = {0, 1, 2, 3};
    long cases = 0;
    do {
        for (int c = 0; c < 256; c++) {
            const size_t count[4] = {counts[c & 3], counts[(c >> 2) & 3], counts[(c >> 4) & 3], counts[(c >> 6) & 3]};
            if (check_case(order, count)) return 1;
            cases++;
        }
    } while (std::next_permutation(order, order + 4));
    printf("layout_check ok: %ld cases\n", cases);
    return 0;
}
