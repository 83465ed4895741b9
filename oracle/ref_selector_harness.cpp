/* ref_selector_harness.cpp -- runs the REFERENCE'S OWN pixel selector
 * (thirdparty/PixelSelector2.cpp: makeHists / select / makeMaps) on caller-given
 * squared-gradient planes.  TEST INFRASTRUCTURE ONLY.
 *
 * The reference's file is compiled from where it lies (-I<reference>/thirdparty); the
 * headers it asks for beyond the C++ library come from oracle/ref_shim (-I, the
 * project's own stand-ins).  Nothing of the reference is copied here.
 *
 * Two things are observed rather than returned by the reference:
 *   - ths / thsSmoothed are private members: `private` is opened for the include;
 *   - the potential of each selection pass: select() clears the map once per pass
 *     (its memset of map_out), and that call is routed through note_memset(), which
 *     writes down currentPotential at that moment.
 */
#include <cstring>
#include <cstdlib>
#include <cmath>
#include <vector>
#include <algorithm>
#include <cassert>
#include <cstdio>

#define private public
#include <PixelSelector2.h>
#undef private

namespace {
dso::PixelSelector *g_sel = nullptr;
const void *g_map = nullptr;
int g_pots[4];
int g_npass = 0;

void *note_memset(void *p, int c, size_t n)
{
    if (p == g_map && g_sel) {
        if (g_npass < 4) g_pots[g_npass] = g_sel->currentPotential;
        ++g_npass;
    }
    return std::memset(p, c, n);
}
}   // namespace

#define memset note_memset
#include <PixelSelector2.cpp>
#undef memset

namespace {
void fill_frame(cvo::frame &fr, std::vector<Eigen::Vector3f> &dI, int w, int h, const float *ag0, const float *ag1,
                const float *ag2)
{
    dI.assign((size_t)w * h, Eigen::Vector3f(0.f, 0.f, 0.f));   /* read by select(), never used */
    fr.frame_id = 0;
    fr.w = w;
    fr.h = h;
    fr.dI = dI.data();
    for (int l = 0; l < PYR_LEVELS; ++l) fr.dI_pyr[l] = nullptr;
    fr.dI_pyr[0] = fr.dI;
    fr.abs_squared_grad[0] = const_cast<float *>(ag0);
    fr.abs_squared_grad[1] = const_cast<float *>(ag1);
    fr.abs_squared_grad[2] = const_cast<float *>(ag2);
    fr.avg_abs_squared_grad = 0.f;
}

void define_unwritten_cells(dso::PixelSelector &sel, int w, int h)
{
    const int ncell = (w / 32) * (h / 32);
    if (ncell > 0)
        for (int i = 0; i < 100; ++i) sel.thsSmoothed[ncell + i] = sel.thsSmoothed[ncell - 1];
}
}   // namespace

/* One selection pass of the reference at a given potential, before any sub-sampling
 * (what the census of tests/selector_ref_cases.py looks at): makeHists, the unwritten
 * cells defined or not as below, then select().  n_out[3]: picks of level 0 / 1 / 2. */
extern "C" void ref_selector_select(int w, int h, const float *ag0, const float *ag1, const float *ag2, int pot,
                                    int define_unwritten, float *map_out, int *n_out)
{
    cvo::frame fr;
    std::vector<Eigen::Vector3f> dI;
    fill_frame(fr, dI, w, h, ag0, ag1, ag2);
    dso::PixelSelector sel(w, h);
    sel.makeHists(&fr);
    if (define_unwritten) define_unwritten_cells(sel, w, h);
    const Eigen::Vector3i n = sel.select(&fr, map_out, pot, 1.0f);
    for (int k = 0; k < 3; ++k) n_out[k] = n[k];
}

/* map_out: w*h floats; ths_out, ths_smoothed_out: (w/32)*(h/32) floats each;
 * pots_out[2]: the potential of the first and (if *npass_out == 2) second selection
 * pass; *pot_after_out: currentPotential once makeMaps has returned.
 * define_unwritten != 0: makeHists runs first and the 100 slots of thsSmoothed behind
 * the last cell (the slack of its new[], never written by the reference) take the
 * last cell's value before makeMaps; 0: nothing is touched.
 * Returns makeMaps' return value. */
extern "C" int ref_selector_make_maps(int w, int h, const float *ag0, const float *ag1, const float *ag2,
                                      float density, int define_unwritten, float *map_out, float *ths_out,
                                      float *ths_smoothed_out, int *pots_out, int *npass_out, int *pot_after_out)
{
    cvo::frame fr;
    std::vector<Eigen::Vector3f> dI;
    fill_frame(fr, dI, w, h, ag0, ag1, ag2);
    dso::PixelSelector sel(w, h);
    const int ncell = (w / 32) * (h / 32);
    if (define_unwritten) {
        sel.makeHists(&fr);
        define_unwritten_cells(sel, w, h);
    }
    g_sel = &sel;
    g_map = map_out;
    g_npass = 0;
    const int ret = sel.makeMaps(&fr, map_out, density);
    g_sel = nullptr;
    g_map = nullptr;
    for (int i = 0; i < ncell; ++i) {
        ths_out[i] = sel.ths[i];
        ths_smoothed_out[i] = sel.thsSmoothed[i];
    }
    pots_out[0] = g_pots[0];
    pots_out[1] = g_npass > 1 ? g_pots[1] : g_pots[0];
    *npass_out = g_npass;
    *pot_after_out = sel.currentPotential;
    return ret;
}
