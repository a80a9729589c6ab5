// rs_arena.h — the one walker over a caller-owned workspace (host only, plain C++: no HIP include).
//
// Every entry point has ONE layout function that takes its dimensions and an rs_arena& and fills a struct of typed pointers.
// The *_workspace_bytes query runs it on an arena without a base (it measures: every pointer is null), the launch runs the
// same function on the caller's pointer (it carves), and both read the size from bytes(): the two cannot disagree.
// Layout arithmetic that more than one layout function shares (rs_sub_chunk_rule) lives here too, where g++ can test it.
#pragma once
#include <stddef.h>

static inline size_t rs_align(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

struct rs_arena {
    char* base;          // nullptr: measure only
    size_t offset = 0;
    explicit rs_arena(void* workspace = nullptr) : base(static_cast<char*>(workspace)) {}
    // n_elems elements of T at the running offset (null when measuring); the offset moves on by the 256-byte aligned extent,
    // so a piece of no elements takes no room and consecutive pieces are adjacent up to that alignment
    template <typename T>
    T* take(size_t n_elems) {
        T* p = base ? reinterpret_cast<T*>(base + offset) : nullptr;
        offset += rs_align(n_elems * sizeof(T));
        return p;
    }
    size_t bytes() const { return offset; }
};

// Conv2dSubsampling runs in chunks of utterances.  per_utt = bytes of the chunked buffer per utterance, bound = what a chunk of it may
// hold, grid_rows = rows per utterance of the chunked kernels' grid (limit 65535) -> chunk = utterances per pass (1 .. B), reserve =
// bytes to set aside for the buffer.  The reserve is the chunk's BOUND, not chunk * per_utt: floor(bound / per_utt) * per_utt goes up
// and down with the length, and a caller that allocates for its longest geometry and runs shorter ones in the same workspace
// (rs_workspace_bytes is asked once per buffer set) must never be told that a shorter batch needs more.
struct rs_sub_chunk { int chunk; size_t reserve; };
static inline rs_sub_chunk rs_sub_chunk_rule(size_t per_utt, size_t bound, size_t grid_rows, int B) {
    size_t chunk = bound / per_utt;
    if (chunk < 1) chunk = 1;
    if (chunk > (size_t)B) chunk = (size_t)B;
    while (chunk > 1 && chunk * grid_rows > 65535) --chunk;
    const size_t most = (size_t)B * per_utt < bound ? (size_t)B * per_utt : bound;
    return {(int)chunk, most > per_utt ? most : per_utt};
}
