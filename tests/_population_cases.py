"""The populations and crashed / alive patterns at which the image drivers' launch geometry changes (DESIGN.md sections 27, 28 and 29):
the pattern functions and the case tables that tests/test_gpu_image_populations.py (device against host entry) and the CPU rule tests
(host entry against mirror: test_world_rule.py, test_memory_rule.py, test_qcnn_rule.py) share.  No test and no fixture lives here."""
import numpy as np

# The kernels' population constants, restated; tests/test_qcnn_rule.py and tests/test_memory_rule.py assert the ones _capi.py exposes.
LIST_THREADS = 256    # okWorldListKernel's one workgroup (ok_world.h: __launch_bounds__(256)): a pass of its loop takes 256 agents
WAVE = 64             # a wave of it: the ballot's width (its sums[4] holds LIST_THREADS / WAVE counts)
MEMORY_ROWS = 128     # ok_memory.h: kMemRows, the list slots of a workgroup of okMemoryLayerKernel
MEMORY_WAVE_ROWS = 16  # ok_memory.h: kMemRows / kMemWaves, the row tile of one of its 8 waves
REPLAY_THREADS = 256  # ok_dqn.h: kReplayThreads, the agents of a workgroup of the ring's count and rank kernels
HEAD_SLOTS = 4        # ok_world.h: kWorldHeadSlots, ok_memory.h: kMemHeadSlots, the list slots of a workgroup of the head kernels
HEAD_AGENTS = 16      # ok_world.h: kWorldAgents, ok_conv.h: kConvAgents, the agents of a workgroup of the MFMA heads


def _flags(N, crashed):
    out = np.zeros(N, np.uint8)
    out[crashed] = 1
    return out


# name -> (the fewest agents the pattern needs, N -> the crashed flags [N] uint8)
PATTERNS = {
    "none": (1, lambda N: _flags(N, slice(0, 0))),
    "all": (1, lambda N: _flags(N, slice(None))),
    "first_only_alive": (2, lambda N: _flags(N, slice(1, None))),
    "last_only_alive": (2, lambda N: _flags(N, slice(0, N - 1))),
    "alternate": (2, lambda N: _flags(N, slice(1, None, 2))),  # every second agent: 1, 3, 5, ...
    "wave1_gone": (2 * WAVE, lambda N: _flags(N, slice(WAVE, 2 * WAVE))),
    "pass0_gone": (LIST_THREADS, lambda N: _flags(N, slice(0, LIST_THREADS))),
    "random30": (1, lambda N: (np.random.default_rng(3000 + N).random(N) < 0.3).astype(np.uint8)),
}


def fits(pattern, N):
    return N >= PATTERNS[pattern][0]


def crashed(pattern, N):
    """The crashed flags [N] uint8 of a pattern that fits N."""
    assert fits(pattern, N), (pattern, N)
    out = PATTERNS[pattern][1](N)
    assert out.dtype == np.uint8 and out.shape == (N,)
    return out


# ---- a. the world act: (shape, N, skip_crashed, pattern) -----------------------------------------------------------------------------
# N: one full wave of the list kernel; a second wave with one agent; one full pass; a second pass with one agent; a third, partial pass
WORLD_COUNTS = (64, 65, 256, 257, 600)
WORLD_CASES = [("tiny", N, skip, p) for N in WORLD_COUNTS for skip, p in [(0, "random30")] + [(1, p) for p in PATTERNS if fits(p, N)]]
WORLD_CASES.append(("ragged", 257, 1, "random30"))  # K blocks and idle waves with a list that is not the identity

# ---- b. the memory act: (shape, N, carry, skip_crashed, pattern) ---------------------------------------------------------------------
# N: wave 7 of the layer kernel partial; all eight waves full; a second row workgroup of one row; three row workgroups
MEMORY_COUNTS = (113, 128, 129, 257)
MEMORY_PATTERNS = [(0, "none")] + [(1, p) for p in ("alternate", "wave1_gone", "last_only_alive", "all", "random30")]
MEMORY_CASES = [(name, N, 1, skip, p) for name in ("h16", "z128") for N in MEMORY_COUNTS for skip, p in MEMORY_PATTERNS if fits(p, N)]
MEMORY_CASES.append(("h16", 129, 0, 1, "random30"))  # carry == 0
# several column blocks against a second row workgroup.  h48 (two column blocks, the last with one live tile) stands where h512 (sixteen)
# was meant to: the host entry takes 3.2 s an act for 129 agents of h512, two acts a case, against 1.3 s for h48
MEMORY_CASES.append(("h48", 129, 1, 0, "none"))

# ---- c. the frame ring: (network shape, N, selection, capacity) ----------------------------------------------------------------------
# selection -> (N, push) -> the alive flags [N] uint8 of that push, or None for OK_REPLAY_PUSH_ALL
def _seeded(share):
    return lambda N, push: (np.random.default_rng(4000 + 10 * N + push).random(N) < share).astype(np.uint8)


def _only(agents):
    return lambda N, push: _flags(N, list(agents))


SELECTIONS = {
    "all": lambda N, push: np.ones(N, np.uint8),
    "alive70_of_random30": lambda N, push: (np.random.default_rng(3000 + N + push).random(N) >= 0.3).astype(np.uint8),  # random30's alive agents
    "alive70": _seeded(0.7),
    "group1_gone": lambda N, push: 1 - _flags(N, slice(REPLAY_THREADS, 2 * REPLAY_THREADS)),  # workgroup 1 of 0 .. 2 counts nothing
    "four_corners": _only((0, REPLAY_THREADS - 1, REPLAY_THREADS, 4 * REPLAY_THREADS)),  # one agent in workgroup 4, none in 2 and 3
    "push_all": lambda N, push: None,
    "nobody": lambda N, push: np.zeros(N, np.uint8),
}
RING_CASES = [
    ("tiny", 65, "all", 40),                       # a second wave of one agent; wraps on the first push (n > C)
    ("tiny", 256, "alive70_of_random30", 1000),    # one full workgroup; three pushes of about 180, nothing wraps
    ("tiny", 257, "all", 600),                     # a second workgroup of one agent; wraps on the third push
    ("tiny", 600, "alive70", 100),                 # n > C: the last 100 selected agents lie in workgroups 1 and 2
    ("tiny", 600, "group1_gone", 4096),            # a workgroup whose count is 0 between two that are not
    ("tiny", 1025, "four_corners", 8),             # ranks 0 .. 3 from workgroups 0, 0, 1 and 4
    ("tiny", 1025, "push_all", 8),                 # n = 1025 > C = 8: the survivors are the last workgroups' agents
    ("tiny", 1025, "nobody", 40),                  # the empty selection: `pushed` and the ring stay as they are
    ("odd", 257, "alive70", 600),                  # the planes moved float by float
]
RING_PUSHES = 3


def ring_inputs(S, A, N, selection, push, rays):
    """One push's host arrays: action, alive (None: PUSH_ALL), frames, next_frames, crashed, reward, dist [N][rays]."""
    rng = np.random.default_rng(6000 + 10 * N + push)
    return dict(action=rng.integers(0, A, N).astype(np.int64), alive=SELECTIONS[selection](N, push),
                frames=rng.integers(0, 256, (N, S, S, 4), dtype=np.uint8), next_frames=rng.integers(0, 256, (N, S, S, 4), dtype=np.uint8),
                crashed=(rng.random(N) < 0.3).astype(np.uint8), reward=rng.normal(size=N).astype(np.float32),
                dist=rng.uniform(0.5, 250.0, (N, rays)).astype(np.float32))


# ---- the CPU side: the host entries against the slow mirrors ------------------------------------------------------------------------------
HOST_N = 129                               # a second row workgroup of the memory's layer kernel, a third wave of the list kernel
HOST_PATTERNS = ("alternate", "wave1_gone")
HOST_MIRRORED = (0, 1, 63, 64, 65, 127, 128)  # the agents the mirror is run for: both sides of every wave's edge and the last one
