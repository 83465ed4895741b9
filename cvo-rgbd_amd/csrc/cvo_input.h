// cvo_input.h -- the arithmetic on a caller's image that the front end does before anything is enqueued: is the pitch
// one an image of this row can have, where does the image's last byte lie, does it lie inside an allocation.  Pure C++,
// no device and no runtime: cvo_frontend.hip and cvo_depthfmt.hip use it, and tests/cpp/input_extent_host.cpp drives
// it on the host.  Nothing here overflows for strides up to SIZE_MAX: a product is formed only after a division has
// shown that it fits.
#ifndef CVO_INPUT_H
#define CVO_INPUT_H

#include <stddef.h>
#include <stdint.h>

// a pitch an image of `row_bytes` per row and values of `item` bytes can have: at least the row, a multiple of the item
inline bool input_stride_ok(size_t stride, size_t row_bytes, size_t item)
{
    return item > 0 && stride >= row_bytes && stride % item == 0;
}

// *extent = (rows - 1) * stride + row_bytes, the bytes from the image's first to one past its last; false (and
// *extent untouched) where rows < 1 or that number does not fit a size_t
inline bool input_extent(size_t rows, size_t stride, size_t row_bytes, size_t *extent)
{
    if (rows < 1) return false;
    const size_t gaps = rows - 1;
    if (gaps != 0 && stride > (SIZE_MAX - row_bytes) / gaps) return false;
    *extent = gaps * stride + row_bytes;
    return true;
}

// an image that begins `offset` bytes into an allocation of `size` bytes ends inside it
inline bool input_fits(size_t offset, size_t size, size_t rows, size_t stride, size_t row_bytes)
{
    size_t extent = 0;
    if (!input_extent(rows, stride, row_bytes, &extent)) return false;
    return offset <= size && extent <= size - offset;
}

#endif
