// cvo_lidar_stage.h -- a scan as it is staged for the device, and the host code that packs it.  Host only, standard C++
// alone: cvo_frontend.hip includes it, and so does tests/cpp/lidar_stage_host.cpp, which drives it under the host
// compiler's sanitizers.
//
// A staged scan is a header of FE_LIDAR_HEADER bytes and behind it the records, packed:
//   word 0        int32 n, the number of points of this frame
//   words 1..3    0
//   words 4..9    float twist[6] of this frame (w then v: cvo_fe_set_lidar_motion); 0 without a sweep
//   words 10..11  0
// A record is x y z (12 bytes), or x y z and the raw time word of the caller's record (16 bytes) under a field mode of
// the sweep contract (include/cvo_frontend.h at cvo_fe_lidar_sweep).  The header is a multiple of 16 bytes, so that the
// 16-byte records are aligned where the allocation is.
#ifndef CVO_LIDAR_STAGE_H
#define CVO_LIDAR_STAGE_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

constexpr int FE_LIDAR_HEADER = 48;       // bytes in front of the packed records
constexpr int FE_LIDAR_TWIST_WORD = 4;    // the header's word where the frame's twist begins

// bytes of one staged record: `time_offset` is the byte offset of the time word in the caller's record, < 0: none
inline size_t lidar_record_bytes(int time_offset) { return time_offset >= 0 ? 16 : 12; }

inline size_t lidar_scan_bytes(int capacity, size_t record)
{
    return (size_t)FE_LIDAR_HEADER + (size_t)capacity * record;
}

// `n` points of records `stride` bytes apart into a scan's staging: the count and the twist (NULL: zero) in the header,
// the records packed.  Reads bytes [0, 12) of every record and, with time_offset >= 0, [time_offset, time_offset + 4):
// the caller has checked 12 <= stride and time_offset + 4 <= stride.  Writes lidar_scan_bytes(n, record) bytes.
inline void lidar_stage(uint8_t *scan, const void *points, size_t stride, int n, int time_offset, const float *twist)
{
    int32_t header[FE_LIDAR_HEADER / 4] = {n};
    if (twist) memcpy(header + FE_LIDAR_TWIST_WORD, twist, 6 * sizeof(float));
    memcpy(scan, header, sizeof(header));
    uint8_t *dst = scan + FE_LIDAR_HEADER;
    const uint8_t *src = (const uint8_t *)points;
    if (time_offset < 0) {
        if (stride == 12) {
            if (n) memcpy(dst, src, (size_t)n * 12);
            return;
        }
        for (int i = 0; i < n; ++i) memcpy(dst + (size_t)i * 12, src + (size_t)i * stride, 12);
        return;
    }
    if (stride == 16 && time_offset == 12) {
        if (n) memcpy(dst, src, (size_t)n * 16);
        return;
    }
    for (int i = 0; i < n; ++i) {
        memcpy(dst + (size_t)i * 16, src + (size_t)i * stride, 12);
        memcpy(dst + (size_t)i * 16 + 12, src + (size_t)i * stride + (size_t)time_offset, 4);
    }
}

#endif
