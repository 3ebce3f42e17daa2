// ethcnn_tile_table.hip -- k0 over a TABLE of pictures: the CTU-load stage of ethcnn_tile.hip for up to 32 pictures of different
// sizes in one launch (the front-end of ethcnn_ldp_sessions_step: one frame each of several live encoders).  Segment j of the table
// owns the global 16-CTU groups [first_group_j, first_group_j + ceil(n_total_j / 16)): every segment starts on a group boundary, so
// a block = one global group belongs to exactly one picture and runs that picture's tile_group (ethcnn_tile_group.h) unchanged,
// with the record bases moved so that local group g lands at the global group.  The lanes of a short last group beyond n_total_j
// get zero records: the trunk and FC1 compute rows for them that nothing reads.  Bytes only: 4096 B/CTU in, 6656 B/CTU out.
#include <hip/hip_runtime.h>

#include "ethcnn_kernels.h"
#include "ethcnn_tile_group.h"

namespace ethcnn {

__global__ __launch_bounds__(256) void k0_tile_table(const TileTable tab, int group0, uint4* __restrict__ XS, uint4* __restrict__ XM,
                                                     uint4* __restrict__ XL) {
    __shared__ uint32_t tile[16 * kSlabCtuPitch];
    const int G = group0 + (int)blockIdx.x;  // uniform: the table walk below is scalar
    int j = 0;
    for (int i = 1; i < tab.nseg; ++i)
        if (tab.seg[i].first_group <= G) j = i;
    const TileSeg sg = tab.seg[j];
    const int grp = G - sg.first_group;
    // tile_group stores local group grp at base + grp * (4096 | 2048 | 512) records; the pass's buffers begin at global group group0.
    // (Negative for a picture that began in the pass before: the sum with grp is this block's index, 0 <= blockIdx.x < ngroups.)
    const long shift = (long)sg.first_group - group0;
    uint4* const xs = XS + shift * 4096;
    uint4* const xm = XM + shift * 2048;
    uint4* const xl = XL + shift * 512;
    if (sg.fast)
        tile_group<true, false, false>(tile, sg.luma, sg.width, sg.height, sg.pitch, sg.frame_stride, sg.cw, sg.nctu, 0, sg.n_total, grp, xs, xm, xl);
    else
        tile_group<false, false, false>(tile, sg.luma, sg.width, sg.height, sg.pitch, sg.frame_stride, sg.cw, sg.nctu, 0, sg.n_total, grp, xs, xm, xl);
}

TileSeg tile_seg(const uint8_t* d_luma, const FrameGeom& g, int n_total, int first_group) {
    const bool fast = (g.width % 16 == 0) && (g.pitch % 16 == 0) && (g.frame_stride % 16 == 0) && (reinterpret_cast<uintptr_t>(d_luma) % 16 == 0);
    return TileSeg{d_luma, g.width, g.height, g.pitch, g.frame_stride, g.cw, g.nctu, n_total, first_group, fast ? 1 : 0};
}

void launch_tile_table(const TileTable& t, int group0, int ngroups, const Workspace& ws, hipStream_t s) {
    hipLaunchKernelGGL(k0_tile_table, dim3(ngroups), dim3(256), 0, s, t, group0, ws.xs, ws.xm, ws.xl);
}

}  // namespace ethcnn
