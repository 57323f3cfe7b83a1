"""The committed slices of the differential campaigns that tests/test_gpu_differential.py runs on every GPU test run.

The seeds were picked once, by scanning the campaigns' make_case on the CPU for what the slice must cover (tests/test_differential_
checkers.py::test_slices_cover asserts it), and all lie in the seed ranges of the committed campaign records: a failure on one of them
is a regression since then.
  ENGINE_SEEDS        profiles/r06/fuzz_engines_s10000.txt (seeds 10000 ... 13999; five polygon cases added for the fused filter
                      on polygons, whose thresholds drop most instances of the others)
  ENGINE_TINY_SEEDS   profiles/r06/fuzz_engines_tiny.txt (seeds 20000 ... 21499, make_case(seed, tiny=True))
  POINT_SEEDS         profiles/r06/fuzz_points.txt (0 ... 2999)
  ANNOTATION_SEEDS    profiles/r06/fuzz_annotations.txt (0 ... 3999)
  AUX_SEEDS           profiles/r06/fuzz_aux.txt (0 ... 1999)
  HULL_SEEDS          profiles/hull/fuzz_hull.txt (oracle/campaigns/hull.py: the convex-hull yaw of the depth + mask fit; seeds
                      70000 ... 70499: the whole range has run - 500 cases, 5518 instances, 4277 calls, no failure)
  CLOUD_SEEDS         profiles/clouds/fuzz_clouds.txt (oracle/campaigns/clouds.py: the instance point clouds; seeds 80000 ... 80499:
                      the whole range has run, see the record)
  FORMAT_SEEDS        profiles/formats/fuzz_formats.txt (oracle/campaigns/formats.py: the mask, logit and label packers and the 16-bit
                      depth packers; seeds 90000 ... 90499: the whole range has run, see the record)
  ALIGN_RANSAC_SEEDS  profiles/align_ransac/fuzz_align_ransac.txt (oracle/campaigns/align_ransac.py: the batched RANSAC scale fit, its
                      device draw and the chain select -> fit -> apply; seeds 100000 ... 100499: the whole range has run, see the
                      record)"""

ENGINE_SEEDS = [
    10018, 10023, 10025, 10032, 10034, 10046, 10050, 10051, 10056, 10058,
    10066, 10075, 10078, 10082, 10083, 10086, 10088, 10089, 10094, 10103,
    10170, 10174, 10244, 10284, 10350, 10357, 10424, 10529, 10559, 10571,
    10671, 10790, 10875, 10901, 11041, 11051, 11327, 11373, 11418, 11420,
    11549, 11791, 11812, 11872, 11990,
]

ENGINE_TINY_SEEDS = [
    20007, 20008, 20010, 20016, 20017, 20018, 20022, 20025, 20026, 20028,
    20030, 20043, 20044, 20049, 20055, 20068, 20082, 20105, 20143, 20171,
    20192, 20228, 20243, 20278, 20279, 20350, 20406, 20408, 20413, 20473,
    20560, 20610, 20756, 20808, 21082, 21136, 21209, 21226, 21326, 21369,
]

# seeds of ENGINE_SEEDS with an instance whose footprint is ill-conditioned for raw second moments (kappa > 2^17: the second
# moments pass about the mean decides its axis)
KAPPA_SEEDS = [10023, 10571]

POINT_SEEDS = list(range(40))
ANNOTATION_SEEDS = list(range(40))
AUX_SEEDS = list(range(36)) + [41, 43, 45, 48]   # (41 / 48: one-row frames, 43 / 45: one-column frames)

# the convex-hull campaign (oracle/campaigns/hull.py): every frame class, every refusal reason of full-mask mode, candidate counts of
# 2047 ... 2050, active-tile counts of room - 1 / room / room + 1 on every tiled frame, B = 161 / 300
HULL_SEEDS = [
    70007, 70011, 70015, 70018, 70037, 70038, 70043, 70080, 70101, 70103,
    70106, 70110, 70112, 70125, 70132, 70134, 70143, 70145, 70161, 70169,
    70173, 70179, 70194, 70195, 70199, 70202, 70207, 70208, 70209, 70213,
    70218, 70225, 70235, 70237, 70244, 70246, 70262, 70268, 70279, 70285,
    70329, 70350, 70354, 70368, 70380, 70386, 70404, 70405, 70411, 70432,
    70450, 70452, 70455, 70456, 70469, 70470, 70475, 70483, 70487, 70493,
]

# the campaign of the instance point clouds (oracle/campaigns/clouds.py), picked by a CPU scan of seeds 80000 ... 80499: bands of 1024
# words (all set, the last word short, fewer than 32 pixels over the whole table), a band count BAND_PIX dictates, scan chunks 1 / 2 / 3
# (B = 1025, 2049, 2500; 80013: B = 2049 on 33 x 47), both u8 forms within one instance (1000 x 1), empty instances first / last /
# between and an all-empty case, subsample mode under every run with ranks outside the cloud and instances of exactly 500 / 501 pixels,
# C-entry frame widths of 1 and more than 64 columns below W, mixed sizes, a shared K with an image_index, every frame of the generator
# (tests/test_differential_checkers.py::test_cloud_slice_covers asserts all of it)
CLOUD_SEEDS = [
    80000, 80001, 80002, 80003, 80004, 80005, 80006, 80007, 80008, 80009,
    80010, 80011, 80012, 80013, 80014, 80015, 80016, 80017, 80018, 80019,
    80020, 80021, 80022, 80023, 80024, 80025, 80026, 80027, 80028, 80029,
    80030, 80032, 80033, 80034, 80035, 80036, 80037, 80038, 80039, 80040,
    80041, 80042, 80061, 80068, 80136, 80138, 80231, 80340,
]

# the campaign of the format converters (oracle/campaigns/formats.py), picked by a CPU scan of seeds 90000 ... 90499: every frame of the
# generator - the second trips of the vector packer (129 / 258 / 516 x 512 for f32 / f16, bf16 / u8) and of the general packer (1031 x 509,
# 1025 x 500 padded), the hand-made MaskBits of the unpacker's two-word read, 4194560 x 1 for both depth kernels -, every element kind of
# every packer in a one-size and a mixed case, every threshold, layout, broken input and planted depth value, and a fit leg of more than
# 200 instances (tests/test_differential_checkers.py::test_format_slice_covers asserts all of it).  No group of six takes
# a second on an MI355X (profiles/formats/RESULTS.md), so the large frames stay where the seed order puts them
FORMAT_SEEDS = [
    90000, 90001, 90002, 90003, 90004, 90006, 90007, 90008, 90009, 90010,
    90011, 90013, 90015, 90017, 90018, 90019, 90020, 90021, 90022, 90023,
    90027, 90028, 90030, 90031, 90033, 90034, 90035, 90036, 90037, 90038,
    90039, 90041, 90046, 90047, 90058, 90061, 90103, 90147, 90206, 90225,
    90250, 90272, 90317, 90359, 90403,
]

# the campaign of the batched RANSAC scale fit (oracle/campaigns/align_ransac.py), picked by a CPU scan of seeds 100000 ... 100499: every
# family and status, every listed n (1 ... 20000: frames of 1, 2, 3, 4 and 5 segments), every max_trials, stop_probability and
# min_samples kind, m_cap tight / wide (-1 and in-range garbage behind m) / shorter than one frame's m, even counts whose upper middle
# value differs from the lower one in each of the two medians, thr == 0 frames that fit and that fail, trials with k < 2, with all
# inlier y equal and with sum xx == 0, trial limits of 0 and infinity, early stops and full runs, the draw-only sizes 16384 / 65536 /
# 65537, depth frames of every size with and without mask and of every status; 100063 holds a frame undecided by its trial limit,
# 100283 one by a score tie and one by a slope, 100494 an undecided depth frame (tests/test_differential_checkers.py::test_align_ransac_slice_covers asserts all of it)
ALIGN_RANSAC_SEEDS = [
    100011, 100037, 100043, 100049, 100063, 100080, 100099, 100101, 100106, 100114,
    100124, 100134, 100156, 100170, 100172, 100178, 100186, 100190, 100208, 100209,
    100222, 100231, 100272, 100275, 100283, 100286, 100291, 100294, 100303, 100319,
    100321, 100324, 100330, 100331, 100352, 100361, 100375, 100380, 100390, 100403,
    100413, 100419, 100433, 100444, 100465, 100478, 100494, 100495,
]
