// cvo_photo.h -- the device side of the photometric contract of include/cvo_frontend.h (at cvo_fe_photometric) behind
// one enqueue function: what cvo_frontend.hip (every kind of frame) and cvo_fe_photometric_image (any image) share.
#ifndef CVO_PHOTO_H
#define CVO_PHOTO_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cvo_frontend.h"

// What travels with a frame from the host: copied to the device by the frame's sequence, so a captured frame replays
// under the values of its own submit.
struct FePhotoHeader {
    uint32_t gain[3];   // Q12, clamped: the caller's under CVO_FE_PHOTO_GAIN, else 4096
    uint32_t rearm;     // AUTO: the lock is opened in front of this frame
};

constexpr int FE_PHOTO_SLOTS = 32;

// What stays on the device between frames (AUTO only): zero when the setting is made.
struct FePhotoState {
    // the frame's sums k, M_0, M_1, M_2 in the first four words of each slot, a slot per 128 bytes; zero between frames
    // (k_fe_photo_gain leaves them so)
    unsigned long long acc[FE_PHOTO_SLOTS][16];
    uint32_t G[3];                // the gains k_fe_photo_apply reads
    uint32_t locked;              // the lock is closed: T holds
    uint32_t T[3];
    uint32_t pad_;
    cvo_fe_photometric_frame rec;   // the frame's record, copied back by the frame's sequence
};

// One frame's correction: `images` images (1, or the 2 of a stereo pair) of np = w * h pixels, dense rows, in place.
// Every pointer is device memory from an allocation of its own (so that it starts on 8 bytes).
struct FePhotoArgs {
    uint8_t *img[2];
    int images;
    int w, h;
    const uint16_t *response;     // 3 * 256, or null
    const uint16_t *vignette;     // w * h dense, or null
    const FePhotoHeader *hdr;
    FePhotoState *state;          // read and written under CVO_FE_PHOTO_AUTO only
    cvo_fe_photometric set;
};

// Under AUTO three launches (k_fe_photo_stat on img[0], k_fe_photo_gain, k_fe_photo_apply), else the last alone;
// nothing that waits for the host, no memset: capturable.  The caller has checked the settings
// (cvo_fe_check_photometric) and the sizes.
void fe_photo_enqueue(const FePhotoArgs &a, hipStream_t s);

// the header of a frame: the caller's gains clamped, or 4096
void fe_photo_header(const cvo_fe_photometric &set, const uint32_t gains_q12[3], bool rearm, FePhotoHeader *out);

// the record of a frame without AUTO, which the device does not make
void fe_photo_plain_record(const FePhotoHeader &hdr, cvo_fe_photometric_frame *out);

#endif
