"""TEST INFRASTRUCTURE: where the capped grids of the tool chain's kernels end.  Almost every kernel around the predictor launches
blocks = min(work, k * CUs) and walks the rest in a grid-stride loop, so whatever the loop carries from one trip to the next (an
in-flight slot that falls off the end, LDS staging that the next trip overwrites and the barrier in front of it) runs only when the
input is larger than one trip of the device in hand.  Each function restates one launcher: the LARGEST input that still fits one trip
on a device of `cus` compute units.  A test that means to reach the second trip sizes its input from these and asserts n > cap first
(a condition on the shape, not a measurement); tests/test_gpu_second_trip.py holds one such test per kernel.  csrc = the directory
hevc-complexity-reduction_amd/csrc."""
import re


def cus(ctx):
    """compute units of the device in hand: what the library's launchers size their grids by"""
    m = re.search(r"(\d+) CUs", ctx.device_name)  # "... (gfx950:sramecc+:xnack-, 256 CUs)"
    if m:
        return int(m.group(1))
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def calib_count(cus):
    """k_calib_count, CTUs: csrc/ethcnn_calib.hip:122-123 (launch_count), grid = min(tiles, 4 * cus), a tile = kTile = 64 CTUs
    (csrc/ethcnn_calib.h:23); the loop: ethcnn_calib.hip:46"""
    return 4 * cus * 64


def sim_pack(cus):
    """k_sim_pack, CTUs: csrc/ethcnn_sim.hip:250-251 (launch_pack), grid = min(tiles, 8 * cus), a tile = kThreads = 256 CTUs; the
    loop: ethcnn_sim.hip:29"""
    return 8 * cus * 256


def uncut(cus):
    """k_uncut_inter, CTU-frames: csrc/ethcnn_replay.hip:102 and :114 (blocks_for, launch_uncut), grid = min(ceil(total / 2), 8 * cus),
    kFlight = 2 CTUs a block and trip; the loop: ethcnn_replay.hip:62"""
    return 8 * cus * 2


def cut_ai(cus):
    """k_cut_ai / k_cut_ai16, records: csrc/ethcnn_samples_kernels.hip:229-230 (launch_cut), grid = min(ceil(nrec / 2), 8 * cus), two
    records a block and trip"""
    return 8 * cus * 2


def cut_inter(cus):
    """k_cut_inter, records: csrc/ethcnn_samples_kernels.hip:229-230 (launch_cut), grid = min(nrec, 8 * cus), one record a block and
    trip; the loop: ethcnn_samples_kernels.hip:179"""
    return 8 * cus


def gather(cus):
    """k_gather<uint4> / <uint32_t>, records of one read-back piece: csrc/ethcnn_samples_kernels.hip:249 (launch_gather), grid =
    min(n, 8 * cus), one record a block and trip; the loop: ethcnn_samples_kernels.hip:218.  A piece is at most 64 MB of records
    (kIoBytes, csrc/ethcnn_samples.cpp:13 and :443): a read above that is several launches."""
    return 8 * cus


def lstm_gather(cus):
    """k_lstm_sample_gather, samples: csrc/ethcnn_lstm_samples_kernels.hip:123 and :140 (blocks_for, launch_sample_gather), grid =
    min(m, 8 * cus), one sample a block and trip; the loop: ethcnn_lstm_samples_kernels.hip:75"""
    return 8 * cus


def lstm_repack(cus):
    """k_resi_repack, records of one chunk: csrc/ethcnn_lstm_samples_kernels.hip:133-134 (launch_repack), grid = min(total, 8 * cus)
    with total = n rounded up to kTileCols = 32 (the tail tiles are written as zeros by the same loop), one CTU a block and trip; the
    loop: ethcnn_lstm_samples_kernels.hip:56"""
    return 8 * cus // 32 * 32


def copy16(cus):
    """k_copy16, bytes: csrc/ethcnn_lstm_samples_kernels.hip:156 (launch_copy16), grid = min(ceil(nbytes / 16 / 256), 8 * cus), 256
    lanes of 16 bytes a block and trip; the loop: ethcnn_lstm_samples_kernels.hip:120"""
    return 8 * cus * 256 * 16


def narrow_units(cus):
    """k_narrow_luma, units (one unit = one 64-segment chunk of one row of one frame; a segment = 16 samples, so a row up to 1024
    samples wide is one unit): csrc/ethcnn_narrow.hip:97-98 (launch_narrow), grid = min(ceil(units / 8), 8 * cus), kWaves = 4 waves a
    block, kFlight = 2 units a wave and trip; the loop: ethcnn_narrow.hip:48"""
    return 8 * cus * 4 * 2


NARROW_CHUNK_SAMPLES = 64 * 16  # a row wider than this has chunk > 0 in k_narrow_luma (csrc/ethcnn_narrow.hip:57-59)
