// Stand-alone host program (no HIP, no GPU): every workspace layout of csrc/mi3d_workspace.h is laid over a malloc'ed
// buffer of EXACTLY the size the same walk reports, and the first and the last byte of every array are written.  Built
// with -fsanitize=address,undefined a byte beyond the buffer, a misaligned array or a null offset ends it; without a
// sanitizer it still checks that the arrays lie in the buffer, in ascending order, apart, 8-byte aligned, and that the last
// one ends on the last byte.  The element counts are written out here a second time on purpose: this is the check of the
// one statement in the header.  tests/test_mesh_workspace_cpu.py builds and runs it; it prints one line per layout and
// size, `name nv nt bytes`, which that test compares with the library's queries.
#include <cstdio>
#include <cstdlib>

#include "mi3d_workspace.h"

using namespace mi3d_workspace;

namespace {

struct Buffer {
    char *base, *cursor;
    size_t bytes;
    explicit Buffer(size_t n) : base(static_cast<char *>(std::malloc(n ? n : 1))), cursor(base), bytes(n) {
        if (base == nullptr) std::exit(3);
    }
    ~Buffer() { std::free(base); }
    template <typename T>
    void touch(T *array, size_t count, const char *what) {
        char *first = reinterpret_cast<char *>(array);
        const size_t n = count * sizeof(T);
        if (first < cursor || first + n > base + bytes || (first - base) % 8 != 0) {
            std::fprintf(stderr, "%s: [%td, %td) of %zu bytes, behind %td\n", what, first - base, first + n - base, bytes,
                         cursor - base);
            std::exit(1);
        }
        if (count != 0) {
            array[0] = T();
            array[count - 1] = T();
            first[0] = 1;
            first[n - 1] = 1;
        }
        cursor = first + n;
    }
    void done(const char *what, size_t slack) {  // the last array ends the buffer, but for its own padding
        if (static_cast<size_t>(base + bytes - cursor) > slack) {
            std::fprintf(stderr, "%s: %td bytes unused at the end\n", what, base + bytes - cursor);
            std::exit(1);
        }
    }
};

void walk_mc(uint32_t n) {
    const size_t bytes = bytes_of(mc_layout, n);
    Buffer b(bytes);
    const McWorkspace w = at(b.base, mc_layout, n);
    const size_t nb = blocks_of(n, kLayoutBlock);
    b.touch(w.block_t, nb, "mc block_t");
    b.touch(w.block_v, nb, "mc block_v");
    b.touch(w.first_id, n, "mc first_id");
    b.done("mc", 0);  // the tail is not padded
    std::printf("mc %u 0 %zu\n", n, bytes);
}

void walk_clean(uint32_t nv, uint32_t nt) {
    const size_t bytes = bytes_of(clean_layout, nv, nt);
    Buffer b(bytes);
    const CleanWorkspace w = at(b.base, clean_layout, nv, nt);
    b.touch(w.block_v, blocks_of(nv, kLayoutBlock), "clean block_v");
    b.touch(w.block_t, blocks_of(nt, kLayoutBlock), "clean block_t");
    b.touch(w.flag, nv, "clean flag");
    b.done("clean", 7);
    std::printf("clean %u %u %zu\n", nv, nt, bytes);
}

void walk_simplify(uint32_t nv, uint32_t nt, int shift) {
    const size_t bytes = bytes_of(simplify_layout, nv, nt, shift);
    Buffer b(bytes);
    const SimplifyWorkspace w = at(b.base, simplify_layout, nv, nt, shift);
    const size_t nbv = blocks_of(nv, kLayoutBlock), nbt = blocks_of(nt, kLayoutBlock);
    b.touch(w.table_v, w.cap_v, "simplify table_v");
    b.touch(w.table_t, w.cap_t, "simplify table_t");
    if (reinterpret_cast<char *>(w.acc) != b.base + w.fill_words * 8) std::exit(2);  // the -1 region: the tables
    b.touch(w.acc, (size_t)nv * 4, "simplify acc");
    b.touch(w.ref, nv, "simplify ref");
    if (reinterpret_cast<char *>(w.lead) != b.base + (w.fill_words + w.zero_words) * 8) std::exit(2);  // the zeroed one
    b.touch(w.lead, nv, "simplify lead");
    b.touch(w.tslot, nt, "simplify tslot");
    b.touch(w.block_v, nbv, "simplify block_v");
    b.touch(w.block_t, nbt, "simplify block_t");
    b.touch(w.clusters_v, nbv, "simplify clusters_v");
    b.touch(w.degenerate_t, nbt, "simplify degenerate_t");
    b.touch(w.duplicate_t, nbt, "simplify duplicate_t");
    b.done("simplify", 7);
    std::printf("simplify%d %u %u %zu\n", shift, nv, nt, bytes);
}

void walk_smooth(uint32_t nv, uint32_t nt) {
    const size_t bytes = bytes_of(smooth_layout, nv, nt);
    Buffer b(bytes);
    const SmoothWorkspace w = at(b.base, smooth_layout, nv, nt);
    b.touch(w.cur, nv, "smooth cur");
    b.touch(w.offs, (size_t)nv + 1, "smooth offs");
    b.touch(w.block, blocks_of(nv, kLayoutBlock), "smooth block");
    b.touch(w.moves, nv, "smooth moves");
    b.touch(w.tmp, (size_t)nv * 3, "smooth tmp");
    b.touch(w.pairs, (size_t)nt * 3, "smooth pairs");
    b.done("smooth", 0);
    std::printf("smooth %u %u %zu\n", nv, nt, bytes);
}

void walk_collapse(uint32_t nv, uint32_t nt) {
    const size_t bytes = bytes_of(collapse_layout, nv, nt);
    Buffer b(bytes);
    const CollapseWorkspace w = at(b.base, collapse_layout, nv, nt);
    b.touch(w.ctrl, 1, "collapse ctrl");
    b.touch(w.Q, (size_t)nv * 10, "collapse Q");
    b.touch(w.claim, nv, "collapse claim");
    b.touch(w.keys, (size_t)nt * 3, "collapse keys");
    b.touch(w.P, (size_t)nv * 3, "collapse P");
    b.touch(w.rep, nv, "collapse rep");
    b.touch(w.cur, nv, "collapse cur");
    b.touch(w.offs, (size_t)nv + 1, "collapse offs");
    b.touch(w.blockv, blocks_of(nv, kLayoutBlock), "collapse blockv");
    b.touch(w.tri, (size_t)nt * 3, "collapse tri");
    b.touch(w.rows, (size_t)nt * 3, "collapse rows");
    b.touch(w.xstar, (size_t)nt * 9, "collapse xstar");
    b.touch(w.blockt, blocks_of(nt, kLayoutBlock), "collapse blockt");
    b.touch(w.locked, nv, "collapse locked");
    b.touch(w.alive, nt, "collapse alive");
    b.touch(w.wins, nt, "collapse wins");
    b.done("collapse", 7);
    std::printf("collapse %u %u %zu\n", nv, nt, bytes);
}

}  // namespace

int main() {
    const uint32_t sizes[] = {0, 1, 255, 256, 257, 511, 65537}, dims[] = {2, 3, 5, 17};
    for (uint32_t R : dims) walk_mc(R * R * R);
    for (uint32_t nv : sizes)
        for (uint32_t nt : sizes) {
            walk_clean(nv, nt);
            walk_simplify(nv, nt, 0);
            walk_simplify(nv, nt, 1);
            walk_smooth(nv, nt);
            walk_collapse(nv, nt);
        }
    return 0;
}
