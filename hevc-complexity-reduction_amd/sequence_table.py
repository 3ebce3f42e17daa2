"""The sequence table of the sample extractors (Extract_Data/data_info.py) and their index lists (extract_data_AI.py:19-21,
extract_data_LDP_LDB_RA.py:27-29): data of the interface, restated.  212 4:2:0 files: the first 12 are the raw-image files of the
All-Intra sets, the other 200 are video sequences.  Also what both extractors share: the `--sequences FILE` parser and the
reference's file discovery (glob patterns with its exactly-one-match rule)."""
import glob
import os

import numpy as np

# (name, width, height); the YUV of a sequence is <name>.yuv
SEQUENCES = [
    ('IntraTrain_768x512', 768, 512), ('IntraTrain_1536x1024', 1536, 1024), ('IntraTrain_2880x1920', 2880, 1920),
    ('IntraTrain_4928x3264', 4928, 3264), ('IntraValid_768x512', 768, 512), ('IntraValid_1536x1024', 1536, 1024),
    ('IntraValid_2880x1920', 2880, 1920), ('IntraValid_4928x3264', 4928, 3264), ('IntraTest_768x512', 768, 512),
    ('IntraTest_1536x1024', 1536, 1024), ('IntraTest_2880x1920', 2880, 1920), ('IntraTest_4928x3264', 4928, 3264),
    ('BasketballPass_416x240_50', 416, 240), ('BlowingBubbles_416x240_50', 416, 240), ('BQSquare_416x240_60', 416, 240),
    ('RaceHorses_416x240_30', 416, 240), ('BasketballDrill_832x480_50', 832, 480), ('BQMall_832x480_60', 832, 480),
    ('PartyScene_832x480_50', 832, 480), ('RaceHorses_832x480_30', 832, 480), ('FourPeople_1280x720_60', 1280, 720),
    ('Johnny_1280x720_60', 1280, 720), ('KristenAndSara_1280x720_60', 1280, 720), ('BasketballDrive_1920x1080_50', 1920, 1080),
    ('BQTerrace_1920x1080_60', 1920, 1080), ('Cactus_1920x1080_50', 1920, 1080), ('Kimono_1920x1080_24', 1920, 1080),
    ('ParkScene_1920x1080_24', 1920, 1080), ('PeopleOnStreet_2560x1600_30_crop', 2560, 1600),
    ('Traffic_2560x1600_30_crop', 2560, 1600), ('garden_sif', 352, 240), ('stefan_sif', 352, 240), ('tennis_sif', 352, 240),
    ('tt_sif', 352, 240), ('akiyo_cif', 352, 288), ('bowing_cif', 352, 288), ('bridge_close_cif', 352, 288),
    ('bridge_far_cif', 352, 288), ('bus_cif', 352, 288), ('coastguard_cif', 352, 288), ('container_cif', 352, 288),
    ('deadline_cif', 352, 288), ('flower_cif', 352, 288), ('football_cif', 352, 288), ('foreman_cif', 352, 288),
    ('hall_monitor_cif', 352, 288), ('highway_cif', 352, 288), ('husky_cif', 352, 288), ('mad900_cif', 352, 288),
    ('mobile_cif', 352, 288), ('mother_daughter_cif', 352, 288), ('news_cif', 352, 288), ('pamphlet_cif', 352, 288),
    ('paris_cif', 352, 288), ('sign_irene_cif', 352, 288), ('silent_cif', 352, 288), ('students_cif', 352, 288),
    ('tempete_cif', 352, 288), ('waterfall_cif', 352, 288), ('flower_garden_720x480', 720, 480), ('football_720x480', 720, 480),
    ('galleon_720x480', 720, 480), ('intros_720x480', 720, 480), ('mobile_calendar_720x480', 720, 480),
    ('vtc1nw_720x480', 720, 480), ('washdc_720x480', 720, 480), ('city_4cif', 704, 576), ('crew_4cif', 704, 576),
    ('harbour_4cif', 704, 576), ('ice_4cif', 704, 576), ('soccer_4cif', 704, 576), ('mobcal_ter_720p50', 1280, 720),
    ('parkrun_ter_720p50', 1280, 720), ('shields_ter_720p50', 1280, 720), ('stockholm_ter_720p5994', 1280, 720),
    ('aspen_1080p', 1920, 1080), ('blue_sky_1080p25', 1920, 1080), ('controlled_burn_1080p', 1920, 1080),
    ('crowd_run_1080p50', 1920, 1080), ('dinner_1080p30', 1920, 1080), ('ducks_take_off_1080p50', 1920, 1080),
    ('factory_1080p30', 1920, 1080), ('in_to_tree_1080p50', 1920, 1080), ('life_1080p30', 1920, 1080),
    ('old_town_cross_1080p50', 1920, 1080), ('park_joy_1080p50', 1920, 1080), ('pedestrian_area_1080p25', 1920, 1080),
    ('red_kayak_1080p', 1920, 1080), ('riverbed_1080p25', 1920, 1080), ('rush_field_cuts_1080p', 1920, 1080),
    ('rush_hour_1080p25', 1920, 1080), ('sintel_trailer_2k_1080p24', 1920, 1080), ('snow_mnt_1080p', 1920, 1080),
    ('speed_bag_1080p', 1920, 1080), ('station2_1080p25', 1920, 1080), ('sunflower_1080p25', 1920, 1080),
    ('touchdown_pass_1080p', 1920, 1080), ('tractor_1080p25', 1920, 1080), ('west_wind_easy_1080p', 1920, 1080),
    ('Netflix_Aerial_2048x1080_60fps_420', 2048, 1080), ('Netflix_BarScene_2048x1080_60fps_420', 2048, 1080),
    ('Netflix_Boat_2048x1080_60fps_420', 2048, 1080), ('Netflix_BoxingPractice_2048x1080_60fps_420', 2048, 1080),
    ('Netflix_Crosswalk_2048x1080_60fps_420', 2048, 1080), ('Netflix_Dancers_2048x1080_60fps_420', 2048, 1080),
    ('Netflix_DinnerScene_2048x1080_60fps_420', 2048, 1080), ('Netflix_DrivingPOV_2048x1080_60fps_420', 2048, 1080),
    ('Netflix_FoodMarket_2048x1080_60fps_420', 2048, 1080), ('Netflix_Narrator_2048x1080_60fps_420', 2048, 1080),
    ('Netflix_PierSeaside_2048x1080_60fps_420', 2048, 1080), ('Netflix_RitualDance_2048x1080_60fps_420', 2048, 1080),
    ('Netflix_RollerCoaster_2048x1080_60fps_420', 2048, 1080), ('Netflix_SquareAndTimelapse_2048x1080_60fps_420', 2048, 1080),
    ('Netflix_Tango_2048x1080_60fps_420', 2048, 1080), ('Netflix_ToddlerFountain_2048x1080_60fps_420', 2048, 1080),
    ('Netflix_TunnelFlag_2048x1080_60fps_420', 2048, 1080), ('Netflix_WindAndNature_2048x1080_60fps_420', 2048, 1080),
    ('female150', 1920, 1080), ('male150', 1920, 1080), ('onedarkfinal', 1920, 1080), ('simo', 1920, 1080),
    ('training', 1920, 1080), ('x2', 1920, 1080), ('videoSRC003_640x360_30', 640, 360), ('videoSRC004_640x360_30', 640, 360),
    ('videoSRC005_640x360_30', 640, 360), ('videoSRC008_640x360_30', 640, 360), ('videoSRC009_640x360_30', 640, 360),
    ('videoSRC010_640x360_30', 640, 360), ('videoSRC015_640x360_30', 640, 360), ('videoSRC016_640x360_30', 640, 360),
    ('videoSRC019_640x360_30', 640, 360), ('videoSRC023_640x360_30', 640, 360), ('videoSRC025_640x360_30', 640, 360),
    ('videoSRC034_640x360_30', 640, 360), ('videoSRC035_640x360_30', 640, 360), ('videoSRC037_640x360_30', 640, 360),
    ('videoSRC050_640x360_30', 640, 360), ('videoSRC056_640x360_30', 640, 360), ('videoSRC062_640x360_30', 640, 360),
    ('videoSRC065_640x360_30', 640, 360), ('videoSRC073_640x360_30', 640, 360), ('videoSRC074_640x360_30', 640, 360),
    ('videoSRC075_640x360_30', 640, 360), ('videoSRC078_640x360_30', 640, 360), ('videoSRC079_640x360_30', 640, 360),
    ('videoSRC082_640x360_30', 640, 360), ('videoSRC083_640x360_30', 640, 360), ('videoSRC085_640x360_30', 640, 360),
    ('videoSRC095_640x360_24', 640, 360), ('videoSRC100_640x360_24', 640, 360), ('videoSRC102_640x360_24', 640, 360),
    ('videoSRC104_640x360_24', 640, 360), ('videoSRC107_640x360_24', 640, 360), ('videoSRC109_640x360_24', 640, 360),
    ('videoSRC111_640x360_24', 640, 360), ('videoSRC113_640x360_24', 640, 360), ('videoSRC114_640x360_24', 640, 360),
    ('videoSRC117_640x360_24', 640, 360), ('videoSRC122_640x360_30', 640, 360), ('videoSRC125_640x360_30', 640, 360),
    ('videoSRC130_640x360_30', 640, 360), ('videoSRC135_640x360_30', 640, 360), ('videoSRC136_640x360_24', 640, 360),
    ('videoSRC138_640x360_24', 640, 360), ('videoSRC149_640x360_30', 640, 360), ('videoSRC155_640x360_30', 640, 360),
    ('videoSRC160_640x360_24', 640, 360), ('videoSRC163_640x360_24', 640, 360), ('videoSRC170_640x360_24', 640, 360),
    ('videoSRC176_640x360_24', 640, 360), ('videoSRC180_640x360_24', 640, 360), ('videoSRC182_640x360_24', 640, 360),
    ('videoSRC183_640x360_24', 640, 360), ('videoSRC188_640x360_24', 640, 360), ('videoSRC192_640x360_24', 640, 360),
    ('videoSRC195_640x360_24', 640, 360), ('videoSRC198_640x360_24', 640, 360), ('videoSRC200_640x360_24', 640, 360),
    ('videoSRC201_640x360_24', 640, 360), ('videoSRC204_640x360_24', 640, 360), ('videoSRC213_640x360_24', 640, 360),
    ('Harmonic_2Rally_1_1080p_30', 1920, 1080), ('Harmonic_2Rally_2_1080p_30', 1920, 1080),
    ('Harmonic_3fjords_1_1080p_30', 1920, 1080), ('Harmonic_3fjords_2_1080p_30', 1920, 1080),
    ('Harmonic_5costa_3_1080p_30', 1920, 1080), ('Harmonic_5costa_5_1080p_30', 1920, 1080),
    ('Harmonic_6hongkong_2_1080p_30', 1920, 1080), ('Harmonic_6hongkong_6_1080p_30', 1920, 1080),
    ('Harmonic_7_1_1080p_30', 1920, 1080), ('Harmonic_7_7_1080p_30', 1920, 1080),
    ('Harmonic_8americanfootball_2_1080p_30', 1920, 1080), ('Harmonic_8americanfootball_7_1080p_30', 1920, 1080),
    ('Harmonic_10AsianFusion_2_1080p_30', 1920, 1080), ('Harmonic_10AsianFusion_5_1080p_30', 1920, 1080),
    ('Harmonic_11skateboarding_7_1080p_30', 1920, 1080), ('Harmonic_11skateboarding_9_1080p_30', 1920, 1080),
    ('Harmonic_12redrockvol3_2_1080p_50', 1920, 1080), ('Harmonic_12redrockvol3_5_1080p_50', 1920, 1080),
    ('Harmonic_13redrockvol2_2_1080p_50', 1920, 1080), ('Harmonic_13redrockvol2_9_1080p_50', 1920, 1080),
    ('Harmonic_14airacrobatics_2_1080p_50', 1920, 1080), ('Harmonic_14airacrobatics_3_1080p_50', 1920, 1080),
    ('Harmonic_16raptors_2_1080p_50', 1920, 1080), ('Harmonic_16raptors_3_1080p_50', 1920, 1080),
    ('Harmonic_18ANIMALS_3_1080p_50', 1920, 1080), ('Harmonic_18ANIMALS_11_1080p_50', 1920, 1080),
    ('LiquidAssets_anemone_1080p_30', 1920, 1080), ('LiquidAssets_blackfish_1080p_60', 1920, 1080),
    ('LiquidAssets_boats_1080p_30', 1920, 1080), ('LiquidAssets_diver2_1080p_30', 1920, 1080),
]

QP_LIST = [22, 27, 32, 37]
AI_INDEX = {"train": list(range(0, 4)), "valid": list(range(4, 8)), "test": list(range(8, 12))}
_INTER_VALID = [36, 42, 64, 66, 72, 74, 92, 97, 101, 110]
INTER_INDEX = {"train": [v for v in range(30, 123) if v not in _INTER_VALID], "valid": _INTER_VALID, "test": list(range(12, 30))}
SET_NAMES = {"train": "Train", "valid": "Valid", "test": "Test"}


CHROMA_FORMATS = (400, 420, 422, 444)


def check_format(bit_depth, chroma, where):
    """SystemExit unless (bit_depth, chroma) is a source format of include/ethcnn.h; `where` names the option or line at fault"""
    if not 8 <= bit_depth <= 16:
        raise SystemExit("%s: bit depth %d outside 8..16" % (where, bit_depth))
    if chroma not in CHROMA_FORMATS:
        raise SystemExit("%s: chroma format %d is not one of %s" % (where, chroma, " ".join(str(c) for c in CHROMA_FORMATS)))


def parse_sequences(path, fmt=None):
    """`name width height` per line (blank lines and # comments skipped) -> [(name, width, height)].
    fmt = (bit_depth, chroma), the All-Intra drivers: a line may go on with `bit_depth [chroma]`, which override fmt for that line
    -> [(name, width, height, bit_depth, chroma)]"""
    out = []
    most, form = (3, "`name width height`") if fmt is None else (5, "`name width height [bit_depth [chroma]]`")
    with open(path) as f:
        for n, ln in enumerate(f, 1):
            tok = ln.split("#", 1)[0].split()
            if not tok:
                continue
            if not 3 <= len(tok) <= most or not all(t.isdigit() for t in tok[1:]):
                raise SystemExit("%s:%d: expected %s, got %r" % (path, n, form, ln.rstrip()))
            row = (tok[0], int(tok[1]), int(tok[2]))
            if fmt is not None:
                row += (int(tok[3]) if len(tok) > 3 else fmt[0], int(tok[4]) if len(tok) > 4 else fmt[1])
                check_format(row[3], row[4], "%s:%d" % (path, n))
            out.append(row)
    if not out:
        raise SystemExit("%s: no sequences" % path)
    return out


def find_one(directory, pattern):
    """the reference's discovery rule: glob(directory + pattern) must match exactly one file"""
    hits = glob.glob(os.path.join(directory, pattern))
    if len(hits) != 1:
        raise SystemExit("%s: %d files match %s (exactly one expected)%s" % (directory, len(hits), pattern, "".join("\n  " + h for h in sorted(hits))))
    return hits[0]


def info_file(info_dir, name, qp):
    return find_one(info_dir, "Info*_%s_*qp%d*CUDepth.dat" % (name, qp))


def resi_file(yuv_dir, name, qp):
    return find_one(yuv_dir, "resi*_%s_*qp%d*.yuv" % (name, qp))


def select(sequences_file, index_lists, which, fmt=None):
    """the (name, width, height) list of a set: rows of the table by the set's index list, or every row of a --sequences file.
    fmt = (bit_depth, chroma): rows go on with their source format (parse_sequences)"""
    if sequences_file:
        return parse_sequences(sequences_file, fmt)
    return [SEQUENCES[i] + (() if fmt is None else tuple(fmt)) for i in index_lists[which]]


def ctu_labels(path, w, h, first_frame=0):
    """the 16 depth bytes of every sample a label file yields, [samples, 16] in record order (what the records hold at their label row)"""
    lab = np.fromfile(path, dtype=np.uint8).reshape(-1, h // 16, w // 16)[first_frame:]
    nl, nc = h // 64, w // 64
    return lab[:, :nl * 4, :nc * 4].reshape(-1, nl, 4, nc, 4).transpose(0, 1, 3, 2, 4).reshape(-1, 16)


def add_video_args(ap):
    ap.add_argument("--yuv-dir", help="build the sample sets in HBM from the YUVs here instead of reading --train / --valid files")
    ap.add_argument("--info-dir", help="directory of the Info*_<name>_*qp<QP>*CUDepth.dat label files (with --yuv-dir)")
    ap.add_argument("--sequences", metavar="FILE", help="`name width height` lines: the training sequences (default: the built-in lists)")
    ap.add_argument("--valid-sequences", metavar="FILE", help="the validation sequences (default: --sequences)")


def add_format_args(ap):
    """the All-Intra drivers: the source format of the YUVs (include/ethcnn.h "high-bit-depth and non-4:2:0 sources")"""
    ap.add_argument("--input-bit-depth", type=int, default=8, metavar="N",
                    help="bit depth of the YUVs, 8..16 (above 8: 16-bit little-endian samples); a --sequences line may override it")
    ap.add_argument("--input-chroma-format", type=int, default=420, metavar="{400,420,422,444}",
                    help="chroma format of the YUVs (only luma is read); a --sequences line may override it")


def source_format(a):
    """(bit_depth, chroma) of add_format_args' options; SystemExit on a bad value"""
    check_format(a.input_bit_depth, a.input_chroma_format, "--input-bit-depth / --input-chroma-format")
    return a.input_bit_depth, a.input_chroma_format


def check_source(a):
    if a.yuv_dir or a.info_dir:
        if not (a.yuv_dir and a.info_dir) or a.train or a.valid:
            raise SystemExit("give either --train and --valid, or --yuv-dir and --info-dir")
    elif not (a.train and a.valid):
        raise SystemExit("give --train and --valid (sample files), or --yuv-dir and --info-dir")
