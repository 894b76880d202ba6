// Segment / chunk tables of the layer-wise optimizers (optim_segments.h).
#include "optim_segments.h"

#include <stdexcept>
#include <string>

namespace dcnn {

OptimSegments build_optim_segments(const long* offsets, const long* counts, const unsigned char* no_decay, int params,
                                   bool exclude, long n) {
  OptimSegments t;
  if (params < 0 || n < 0) throw std::invalid_argument("optim_segments: negative size");
  long end = 0;  // first element past the previous slice, rounded up to a block
  for (int i = 0; i < params; ++i) {
    const long off = offsets[i], cnt = counts[i];
    if (off % kSegBlock != 0 || cnt < 0 || off < end)
      throw std::invalid_argument("optim_segments: slice " + std::to_string(i) + " at offset " + std::to_string(off) +
                                  " with " + std::to_string(cnt) + " elements is not " + std::to_string(kSegBlock) +
                                  "-element aligned, or starts before element " + std::to_string(end) +
                                  " where its predecessor ends");
    const long blocks = (cnt + kSegBlock - 1) / kSegBlock;
    if (off + blocks * kSegBlock > n)
      throw std::invalid_argument("optim_segments: slice " + std::to_string(i) + " ends at element " +
                                  std::to_string(off + blocks * kSegBlock) + " of an arena of " + std::to_string(n));
    if ((off + blocks * kSegBlock) / kSegBlock > 0x7fffffffL)
      throw std::invalid_argument("optim_segments: arena of " + std::to_string(n) + " elements is too large");
    const bool flagged = exclude && no_decay && no_decay[i];
    SegInfo s;
    s.first_chunk = (int)t.chunks.size();
    s.adapt = flagged ? 0 : 1;
    s.decay = flagged ? 0 : 1;
    for (long b = 0; b < blocks; b += kSegChunkBlocks) {
      SegChunk c;
      c.first_block = (int)(off / kSegBlock + b);
      c.blocks = (int)(blocks - b < kSegChunkBlocks ? blocks - b : kSegChunkBlocks);
      c.segment = i;
      t.chunks.push_back(c);
    }
    s.chunks = (int)t.chunks.size() - s.first_chunk;
    t.segs.push_back(s);
    end = off + blocks * kSegBlock;
  }
  t.cover = end;
  return t;
}

void check_optim_segments(const SegChunk* chunks, int nchunks, const SegInfo* segs, int nsegs, long n) {
  if (nchunks < 0 || nsegs < 0 || (nchunks && !chunks) || (nsegs && !segs))
    throw std::invalid_argument("optim_segments: " + std::to_string(nchunks) + " chunks, " + std::to_string(nsegs) +
                                " segments: a table is missing");
  for (int c = 0; c < nchunks; ++c) {
    const SegChunk& k = chunks[c];
    if (k.first_block < 0 || k.blocks < 1 || k.blocks > kSegChunkBlocks || k.segment < 0 || k.segment >= nsegs ||
        ((long)k.first_block + k.blocks) * kSegBlock > n)
      throw std::invalid_argument("optim_segments: chunk " + std::to_string(c) + " {first block " +
                                  std::to_string(k.first_block) + ", blocks " + std::to_string(k.blocks) +
                                  ", segment " + std::to_string(k.segment) + "} does not fit " + std::to_string(n) +
                                  " elements in blocks of " + std::to_string(kSegBlock) + ", " +
                                  std::to_string(kSegChunkBlocks) + " blocks a chunk, " + std::to_string(nsegs) +
                                  " segments");
  }
  for (int s = 0; s < nsegs; ++s) {
    const SegInfo& g = segs[s];
    if (g.first_chunk < 0 || g.chunks < 0 || (long)g.first_chunk + g.chunks > nchunks)
      throw std::invalid_argument("optim_segments: segment " + std::to_string(s) + " {first chunk " +
                                  std::to_string(g.first_chunk) + ", chunks " + std::to_string(g.chunks) +
                                  "} lies outside a table of " + std::to_string(nchunks) + " chunks");
  }
}

}  // namespace dcnn
