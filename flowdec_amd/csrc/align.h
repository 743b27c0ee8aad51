// align.h -- fd_align alone, so that the host-only headers (arena.h) get it without the HIP runtime that common.h includes.
#pragma once
#include <stddef.h>

static inline size_t fd_align(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }
