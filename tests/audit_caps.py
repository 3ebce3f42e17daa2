"""TEST INFRASTRUCTURE: where the capped grid of the comparison kernel ends, in the style of tests/grid_caps.py: the LARGEST input that
still fits one trip on a device of `cus` compute units.  A test that means to reach the second trip sizes its input from this and
asserts n > cap first (a condition on the shape, not a measurement).  csrc = the directory hevc-complexity-reduction_amd/csrc."""

TILE = 256  # kTile, csrc/ethcnn_audit.h: CTUs a block stages per trip


def compare(cus):
    """k_compare, CTUs: csrc/ethcnn_audit.h (grid_for), grid = min(tiles, 3 * cus), a tile = kTile = 256 CTUs; the loop:
    csrc/ethcnn_audit.hip, `for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x)`"""
    return 3 * cus * TILE
