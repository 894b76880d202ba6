// Segment / chunk tables of the layer-wise optimizers (LAMB, LARS): the one place both front ends
// and both devices take them from. Plain C++ (no HIP), so the CPU self-tests compile it too.
//
// A flat parameter arena is a row of 64-element aligned slices, one per parameter, with zero gaps.
// A segment is one parameter; a chunk is at most kSegChunkBlocks 64-element blocks of ONE segment.
// Chunks are listed in arena order, so a segment's chunks are a contiguous run of rows. A norm is a
// fixed tree over each chunk's elements and the chunks' partials added in a fixed order over the
// chunk index: it depends on the table only, never on a launch grid.
#pragma once
#include <vector>

namespace dcnn {

constexpr int kSegBlock = 64;        // elements per block (the arena's slice alignment)
constexpr int kSegChunkBlocks = 64;  // blocks per chunk at most: 4096 elements
constexpr int kSegPartFloats = 2;    // floats of partial sums the GPU reduction keeps per chunk (one pair)

struct SegChunk {
  int first_block;  // in 64-element blocks from the arena's start
  int blocks;       // 1 .. kSegChunkBlocks
  int segment;
};

struct SegInfo {
  int first_chunk;
  int chunks;  // 0 for an empty parameter
  int adapt;   // 1: the step is scaled by the trust ratio
  int decay;   // 1: the parameter takes weight decay
};

struct OptimSegments {
  std::vector<SegChunk> chunks;
  std::vector<SegInfo> segs;
  long cover = 0;  // elements the chunks reach: every buffer the kernels touch holds at least this many
};

// offsets / counts: first element and element count of each of the `params` slices, in arena order;
// no_decay: the parameter's exclusion flag (may be null: none flagged); exclude: the optimizer's
// no_decay_norm_bias switch (a flagged parameter then has adapt = decay = 0). n: the arena's size.
// Throws std::invalid_argument naming the numbers for a slice that is not 64-element aligned, that
// overlaps its predecessor, or that ends past n.
OptimSegments build_optim_segments(const long* offsets, const long* counts, const unsigned char* no_decay, int params,
                                   bool exclude, long n);

// What the kernels assume of a table, checked on the host before a launch: every chunk has 1 ..
// kSegChunkBlocks blocks, ends within n elements and names a segment < segs; every segment's run of
// chunks lies within the table. Throws std::invalid_argument naming the numbers.
void check_optim_segments(const SegChunk* chunks, int nchunks, const SegInfo* segs, int nsegs, long n);

}  // namespace dcnn
