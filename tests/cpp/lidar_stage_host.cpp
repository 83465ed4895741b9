// lidar_stage_host.cpp -- lidar_stage of cvo-rgbd_amd/csrc/cvo_lidar_stage.h, the host packing of a scan (the count
// and the frame's twist in the header, the records packed behind it, with or without their time word), driven on its
// own: strides of 12, 16 and 32 bytes, the time word at both ends of the record, no points and a full scan.  Source
// and destination are heap blocks of exactly the bytes the function may read and write, so that a build with
// -fsanitize=address,undefined stops at the first byte beyond either; the contents are compared here.
// Build: g++ -std=c++17 -fsanitize=address,undefined -I cvo-rgbd_amd/csrc lidar_stage_host.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "cvo_lidar_stage.h"

static int failures = 0;

static void expect(bool ok, const char *what, size_t stride, int offset, int n)
{
    if (ok) return;
    std::printf("FAILED %s: stride %zu time_offset %d n %d\n", what, stride, offset, n);
    ++failures;
}

static void run(size_t stride, int offset, int n, const float *twist)
{
    // the last record ends where the allocation ends
    std::unique_ptr<uint8_t[]> src(n ? new uint8_t[(size_t)n * stride] : nullptr);
    for (size_t b = 0; b < (size_t)n * stride; ++b) src[b] = (uint8_t)(b * 37u + 11u);
    const size_t record = lidar_record_bytes(offset), bytes = lidar_scan_bytes(n, record);
    std::unique_ptr<uint8_t[]> dst(new uint8_t[bytes]);
    std::memset(dst.get(), 0xA5, bytes);
    lidar_stage(dst.get(), src.get(), stride, n, offset, twist);
    int32_t header[FE_LIDAR_HEADER / 4];
    std::memcpy(header, dst.get(), sizeof(header));
    expect(header[0] == n && header[1] == 0 && header[2] == 0 && header[3] == 0 && header[10] == 0 && header[11] == 0,
           "the header's count and its unused words", stride, offset, n);
    float got[6];
    std::memcpy(got, header + FE_LIDAR_TWIST_WORD, sizeof(got));
    for (int k = 0; k < 6; ++k) expect(got[k] == (twist ? twist[k] : 0.0f), "the header's twist", stride, offset, n);
    for (int i = 0; i < n; ++i) {
        const uint8_t *d = dst.get() + FE_LIDAR_HEADER + (size_t)i * record, *s = src.get() + (size_t)i * stride;
        expect(std::memcmp(d, s, 12) == 0, "x y z", stride, offset, n);
        if (offset >= 0) expect(std::memcmp(d + 12, s + offset, 4) == 0, "the time word", stride, offset, n);
    }
}

int main()
{
    const float twist[6] = {0.1f, -0.2f, 0.15f, 0.5f, -0.3f, 1.0f};
    const int capacity = 4097;
    int runs = 0;
    for (size_t stride : {(size_t)12, (size_t)16, (size_t)32})
        for (int offset : {-1, 12, (int)stride - 4}) {
            if (offset >= 0 && (offset < 12 || (size_t)offset + 4 > stride)) continue;
            for (int n : {0, 1, capacity})
                for (const float *t : {(const float *)nullptr, twist}) {
                    run(stride, offset, n, t);
                    ++runs;
                }
        }
    static_assert(FE_LIDAR_HEADER % 16 == 0, "the 16-byte records stay aligned behind the header");
    std::printf("%s %d runs\n", failures ? "FAILED" : "ok", runs);
    return failures ? 1 : 0;
}
