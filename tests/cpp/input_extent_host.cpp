// input_extent_host.cpp -- the arithmetic of csrc/cvo_input.h on the host, in a process of its own: what a pitch may be,
// where an image's last byte lies, and whether it lies inside an allocation -- at the sizes at which a product could
// overflow.  Built by tests/test_fe_device_input_cpu.py with the host compiler and -fsanitize=address,undefined
// (unsigned wrap-around is defined, so each case also states the number it expects).
// Prints "ok <cases>" and returns 0, or the first case that failed and 1.
// Build: g++ -std=c++17 -I cvo-rgbd_amd/csrc input_extent_host.cpp
#include <cstdio>
#include <initializer_list>

#include "cvo_input.h"

static int cases = 0;

#define EXPECT(cond)                                                         \
    do {                                                                     \
        ++cases;                                                             \
        if (!(cond)) {                                                       \
            std::printf("failed at line %d: %s\n", __LINE__, #cond);         \
            return 1;                                                        \
        }                                                                    \
    } while (0)

int main()
{
    size_t e = 7;
    // one row: the pitch does not count, however large
    EXPECT(input_extent(1, 0, 10, &e) && e == 10);
    EXPECT(input_extent(1, SIZE_MAX, 10, &e) && e == 10);
    EXPECT(input_extent(1, SIZE_MAX, SIZE_MAX, &e) && e == SIZE_MAX);
    // no rows
    e = 7;
    EXPECT(!input_extent(0, 16, 10, &e) && e == 7);
    // pitch = row
    EXPECT(input_extent(3, 10, 10, &e) && e == 30);
    EXPECT(input_extent(480, 1920, 1920, &e) && e == (size_t)480 * 1920);
    // a pitch further apart
    EXPECT(input_extent(3, 22, 10, &e) && e == 54);
    // pitches near SIZE_MAX / rows: (rows - 1) * pitch + row fits exactly, or does not by one
    for (size_t rows : {(size_t)2, (size_t)3, (size_t)480, (size_t)8192}) {
        const size_t row = 640, gaps = rows - 1;
        const size_t most = (SIZE_MAX - row) / gaps;   // the largest pitch that fits
        EXPECT(input_extent(rows, most, row, &e) && e == gaps * most + row && e >= row);
        e = 7;
        EXPECT(!input_extent(rows, most + 1, row, &e) && e == 7);
        EXPECT(input_extent(rows, most - 1, row, &e) && e == gaps * (most - 1) + row);
        const size_t per_row = SIZE_MAX / rows;        // SIZE_MAX / rows and one either side
        for (size_t pitch : {per_row - 1, per_row, per_row + 1}) {
            const bool fits = pitch <= most;
            e = 7;
            EXPECT(input_extent(rows, pitch, row, &e) == fits && (fits ? e == gaps * pitch + row : e == 7));
        }
        e = 7;
        EXPECT(!input_extent(rows, SIZE_MAX, row, &e) && e == 7);
        EXPECT(!input_fits(0, SIZE_MAX, rows, SIZE_MAX, row));
    }
    // an allocation that ends one byte short of, exactly at and one byte past the image's last byte
    const size_t rows = 5, pitch = 22, row = 10, extent = 4 * 22 + 10;
    EXPECT(!input_fits(0, extent - 1, rows, pitch, row));
    EXPECT(input_fits(0, extent, rows, pitch, row));
    EXPECT(input_fits(0, extent + 1, rows, pitch, row));
    // ... for an image that begins inside the allocation
    EXPECT(!input_fits(6, extent + 5, rows, pitch, row));
    EXPECT(input_fits(6, extent + 6, rows, pitch, row));
    EXPECT(input_fits(6, extent + 7, rows, pitch, row));
    // an offset past the end, and an empty allocation
    EXPECT(!input_fits(extent + 1, extent, rows, pitch, row));
    EXPECT(!input_fits(0, 0, rows, pitch, row));
    EXPECT(!input_fits(SIZE_MAX, SIZE_MAX, 1, 0, 1));
    EXPECT(input_fits(SIZE_MAX - 1, SIZE_MAX, 1, 0, 1));
    // what a pitch may be
    EXPECT(input_stride_ok(10, 10, 1) && input_stride_ok(11, 10, 1) && !input_stride_ok(9, 10, 1));
    EXPECT(input_stride_ok(10, 10, 2) && !input_stride_ok(11, 10, 2) && input_stride_ok(12, 10, 2));
    EXPECT(input_stride_ok(20, 20, 4) && !input_stride_ok(22, 20, 4) && !input_stride_ok(21, 20, 4) && input_stride_ok(24, 20, 4));
    EXPECT(!input_stride_ok(16, 20, 4) && !input_stride_ok(20, 20, 0));
    EXPECT(input_stride_ok(SIZE_MAX, 10, 1) && !input_stride_ok(SIZE_MAX, 10, 2) && input_stride_ok(SIZE_MAX - 1, 10, 2));
    std::printf("ok %d\n", cases);
    return 0;
}
