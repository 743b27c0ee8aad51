// arena.h -- the workspace planner of the forward walk (model.hip: Fwd).  Host-only: no HIP, so that a plain C++ compiler builds it
// alone (tests/c/arena_check.cpp).
#pragma once
#include <stddef.h>

#include <vector>

#include "align.h"

namespace fdm {

// first-fit offset allocator over the caller's workspace; kernels run in stream order so a block may be
// reused as soon as it is released in program order
class Arena {
  struct Blk { size_t off, size; bool free; };
  std::vector<Blk> blks_;
  size_t end_ = 0, peak_ = 0;
 public:
  size_t alloc(size_t bytes) {
    bytes = fd_align(bytes ? bytes : 1);
    for (size_t i = 0; i < blks_.size(); ++i)
      if (blks_[i].free && blks_[i].size >= bytes) {
        const size_t rest = blks_[i].size - bytes;
        blks_[i].free = false; blks_[i].size = bytes;
        if (rest) blks_.insert(blks_.begin() + i + 1, Blk{blks_[i].off + bytes, rest, true});
        return blks_[i].off;
      }
    if (!blks_.empty() && blks_.back().free) {  // grow the trailing free block
      blks_.back().free = false; blks_.back().size = bytes;
      end_ = blks_.back().off + bytes;
    } else {
      blks_.push_back(Blk{end_, bytes, false});
      end_ += bytes;
    }
    if (end_ > peak_) peak_ = end_;
    return blks_.back().off;
  }
  void release(size_t off) {
    for (size_t i = 0; i < blks_.size(); ++i)
      if (blks_[i].off == off && !blks_[i].free) {
        blks_[i].free = true;
        if (i + 1 < blks_.size() && blks_[i + 1].free) { blks_[i].size += blks_[i + 1].size; blks_.erase(blks_.begin() + i + 1); }
        if (i > 0 && blks_[i - 1].free) { blks_[i - 1].size += blks_[i].size; blks_.erase(blks_.begin() + i); }
        if (!blks_.empty() && blks_.back().free) { end_ = blks_.back().off; blks_.pop_back(); }
        return;
      }
  }
  size_t peak() const { return peak_; }
};

}  // namespace fdm
