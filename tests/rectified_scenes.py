"""The scenes the rectified view's scene lists are checked on, shared by the GPU test (the engine runs them) and the host test
(the CPU oracle runs them, to show that no rounded coordinate of theirs lies at a half-integer)."""
SHIPPED_STEPS = 5          # the shipped four-feature scene (slam_helpers.Pair(4, ...)) after this many steps, trajectory saved
MAPPING_SEED, MAPPING_KNOWN, MAPPING_FRAMES, MAPPING_MAX_FEATURES = 7, 12, 24, 24          # mapping_helpers.make_mapping_sequence
