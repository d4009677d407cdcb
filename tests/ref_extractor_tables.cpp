// tests/test_ref_extractor.py: C entry to orbx_build_tables of the HIP-free host unit csrc/orbx_geometry.cpp, so that the
// library's constructor tables can be compared with the compiled reference's without a GPU
#include <cstring>
#include "../orb_slam2_detailed_comments_amd/csrc/orbx_internal.h"

extern "C" void t_build_tables(int nfeatures, float scale_factor, int nlevels, float *scale, float *inv_scale, float *sigma2,
                               float *inv_sigma2, int *nfeat, int *umax16)
{
    orbx_params p;
    std::memset(&p, 0, sizeof p);
    p.nfeatures = nfeatures; p.scale_factor = scale_factor; p.nlevels = nlevels; p.ini_th_fast = 20; p.min_th_fast = 7;
    p.pyramid_mode = ORBX_PYRAMID_FORK_PADDED; p.fp_mode = ORBX_FP_GCC_FMA; p.device = -2; p.max_batch = 1;
    OrbxTables t;
    orbx_build_tables(p, t);
    for (int i = 0; i < nlevels; ++i) {
        scale[i] = t.scale[i]; inv_scale[i] = t.inv_scale[i]; sigma2[i] = t.sigma2[i]; inv_sigma2[i] = t.inv_sigma2[i];
        nfeat[i] = t.nfeat[i];
    }
    for (int i = 0; i < 16; ++i) umax16[i] = t.umax[i];
}
