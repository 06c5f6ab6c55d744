"""The drivers' life cycle on the host ("The drivers' life cycle on the host"): create, num_params, set_params, get_params /
get_state, set_draw_offset, set_greedy and act of the twelve families that attach a network to the handle (actor, DDPG, Gaussian actor,
guided cost learning, lidar transformer, flow matching; the bird's-eye encoder, the image policy, the image Q-net, the world-model
racers, their memory and the image transformer, with the entries only they have: encode, set_epsilon, reset, set_hidden, get_hidden,
embed).  What okenv_last_error says is public API: every refusal's return code and exact text, per entry and in the entry's own order of
checks; the growth and reuse of the vectors, packs, activations and workspaces that are allocated on demand; what a second create
resets; host arrays as parameters."""
import ctypes as C

import numpy as np
import pytest
import torch

import _bev_encoder_numpy as bev_mirror
import _cnn_numpy as cnn_mirror
import _flow_numpy as flow_mirror
import _lidar_numpy as lidar_mirror
import _memory_numpy as memory_mirror
import _qcnn_numpy as qcnn_mirror
import _vit_numpy as vit_mirror
import _world_numpy as world_mirror
from test_gpu_lidar import same  # the predicate of every family's own GPU test: same shape, same bytes
from test_gpu_memory import act_both as memory_act_both, assert_equal as memory_assert_equal, configs as memory_configs, drawn as memory_drawn
from test_gpu_qcnn import config as qcnn_config
from test_gpu_world import RECORD as WORLD_RECORD, host_act as world_host_act, record_tensors as world_record

pytestmark = pytest.mark.gpu
f32 = np.float32
OK, INVALID, STATE = 0, -1, -5
TABLE = ((60.0, 0.0), (30.0, 5.0), (30.0, -5.0))
GCL_WIDTHS = dict(hidden1=8, hidden2=8, cost_hidden1=8, cost_hidden2=8)


def fan(R):
    return np.linspace(-90.0, 90.0, R).astype(f32)


def population(gpu, N, R):
    dev = gpu.BatchedEnvironment.from_track(gpu.Track("Austin"), N, ray_angles_deg=fan(R))
    dev.reset_random(None, 1, 5, 0, 0)
    dev.step(1)
    return dev


@pytest.fixture(scope="module")
def small(gpu):
    """One handle of 3 agents and 3 rays for the refusals of the families: each test touches its own family only (the memory, which
    stands on the racers, has a handle of its own)."""
    dev = population(gpu, 3, 3)
    yield dev
    dev.close()


def refused(dev, handle, rc, code, text):
    """rc is `code`, and okenv_last_error of `handle` (None: the global a NULL handle's message goes to) is exactly `text`."""
    got = dev._L.okenv_last_error(handle).decode()
    assert (rc, got) == (code, text)


# ---- 1. the refusals, per family --------------------------------------------------------------------------------------------------

def test_refusals_actor(gpu, small):
    capi, L, h = gpu.capi, small._L, small._h
    no_value, with_value = capi.actor_params(8, TABLE, 0), capi.actor_params(8, TABLE, 8)
    a, b = C.c_int32(-1), C.c_int32(-1)
    n_pol = 3 * 8 + 8 + 8 * 3 + 3
    buf = np.zeros(n_pol, dtype=f32)
    # a NULL handle
    refused(small, None, L.okenv_actor_create(None, C.byref(with_value)), INVALID, "okenv_actor_create: NULL handle")
    refused(small, None, L.okenv_actor_create(None, None), INVALID, "okenv_actor_create: NULL handle")
    refused(small, None, L.okenv_actor_act(None, None), INVALID, "okenv_actor_act: NULL handle")
    refused(small, None, L.okenv_actor_num_params(None, C.byref(a), C.byref(b)), STATE, "okenv_actor_num_params: call okenv_actor_create first")
    refused(small, None, L.okenv_actor_set_params(None, capi.ptr(buf), None), STATE, "okenv_actor_set_params: call okenv_actor_create first")
    refused(small, None, L.okenv_actor_get_params(None, capi.ptr(buf), None), STATE, "okenv_actor_get_params: call okenv_actor_create first")
    refused(small, None, L.okenv_actor_set_draw_offset(None, None), STATE, "okenv_actor_set_draw_offset: call okenv_actor_create first")
    # before create
    refused(small, h, L.okenv_actor_act(h, None), STATE, "okenv_actor_act: call okenv_actor_create first")
    refused(small, h, L.okenv_actor_num_params(h, C.byref(a), C.byref(b)), STATE, "okenv_actor_num_params: call okenv_actor_create first")
    refused(small, h, L.okenv_actor_num_params(h, None, None), STATE, "okenv_actor_num_params: call okenv_actor_create first")
    refused(small, h, L.okenv_actor_set_params(h, capi.ptr(buf), None), STATE, "okenv_actor_set_params: call okenv_actor_create first")
    refused(small, h, L.okenv_actor_set_params(h, None, None), STATE, "okenv_actor_set_params: call okenv_actor_create first")
    refused(small, h, L.okenv_actor_get_params(h, capi.ptr(buf), None), STATE, "okenv_actor_get_params: call okenv_actor_create first")
    refused(small, h, L.okenv_actor_set_draw_offset(h, None), STATE, "okenv_actor_set_draw_offset: call okenv_actor_create first")
    assert (a.value, b.value) == (-1, -1)
    # created without a value network: a value vector is refused, NULL out pointers and no vector at all are accepted
    assert L.okenv_actor_create(h, C.byref(no_value)) == OK
    assert L.okenv_actor_num_params(h, None, None) == OK and L.okenv_actor_num_params(h, C.byref(a), None) == OK and a.value == n_pol
    assert L.okenv_actor_set_params(h, None, None) == OK
    refused(small, h, L.okenv_actor_set_params(h, capi.ptr(buf), capi.ptr(buf)), INVALID, "okenv_actor_set_params: the actor has no value network")
    refused(small, h, L.okenv_actor_act(h, None), STATE,
            "okenv_actor_act: call okenv_actor_set_params first (every attached network needs its parameters)")
    # created with one: both networks need their parameters
    assert L.okenv_actor_create(h, C.byref(with_value)) == OK
    assert L.okenv_actor_num_params(h, C.byref(a), C.byref(b)) == OK and (a.value, b.value) == (n_pol, 3 * 8 + 8 + 8 + 1)
    value = np.zeros(b.value, dtype=f32)
    refused(small, h, L.okenv_actor_get_params(h, capi.ptr(buf), None), STATE,
            "okenv_actor_get_params: the network has no parameters yet (okenv_actor_set_params)")
    assert L.okenv_actor_get_params(h, None, None) == OK
    assert L.okenv_actor_set_params(h, capi.ptr(buf), None) == OK
    small.sync()
    refused(small, h, L.okenv_actor_get_params(h, capi.ptr(buf), capi.ptr(value)), STATE,
            "okenv_actor_get_params: the network has no parameters yet (okenv_actor_set_params)")
    refused(small, h, L.okenv_actor_act(h, None), STATE,
            "okenv_actor_act: call okenv_actor_set_params first (every attached network needs its parameters)")
    assert L.okenv_actor_set_params(h, None, capi.ptr(value)) == OK
    small.sync()
    assert L.okenv_actor_set_draw_offset(h, None) == OK
    assert L.okenv_actor_act(h, None) == OK  # the gate opens
    small.sync()


def test_refusals_ddpg(gpu, small):
    capi, L, h = gpu.capi, small._L, small._h
    cfg = capi.ddpg_config(8, 8)
    a, b = C.c_int32(-1), C.c_int32(-1)
    st = capi.OkenvDdpgState()
    buf = np.zeros(64, dtype=f32)
    # a NULL handle
    refused(small, None, L.okenv_ddpg_create(None, C.byref(cfg)), INVALID, "okenv_ddpg_create: NULL handle")
    refused(small, None, L.okenv_ddpg_create(None, None), INVALID, "okenv_ddpg_create: NULL handle")
    refused(small, None, L.okenv_ddpg_act(None, None), INVALID, "okenv_ddpg_act: NULL handle")
    refused(small, None, L.okenv_ddpg_num_params(None, C.byref(a), C.byref(b)), STATE, "okenv_ddpg_num_params: call okenv_ddpg_create first")
    refused(small, None, L.okenv_ddpg_set_params(None, capi.ptr(buf), None), STATE, "okenv_ddpg_set_params: call okenv_ddpg_create first")
    refused(small, None, L.okenv_ddpg_get_state(None, C.byref(st)), INVALID, "okenv_ddpg_get_state: NULL argument")
    refused(small, None, L.okenv_ddpg_set_draw_offset(None, None), STATE, "okenv_ddpg_set_draw_offset: call okenv_ddpg_create first")
    # before create
    refused(small, h, L.okenv_ddpg_act(h, None), STATE, "okenv_ddpg_act: call okenv_ddpg_create first")
    refused(small, h, L.okenv_ddpg_num_params(h, None, None), STATE, "okenv_ddpg_num_params: call okenv_ddpg_create first")
    refused(small, h, L.okenv_ddpg_set_params(h, None, None), STATE, "okenv_ddpg_set_params: call okenv_ddpg_create first")
    refused(small, h, L.okenv_ddpg_get_state(h, None), INVALID, "okenv_ddpg_get_state: NULL argument")
    refused(small, h, L.okenv_ddpg_get_state(h, C.byref(st)), STATE,
            "okenv_ddpg_get_state: both networks need their parameters first (okenv_ddpg_create, okenv_ddpg_set_params)")
    refused(small, h, L.okenv_ddpg_set_draw_offset(h, None), STATE, "okenv_ddpg_set_draw_offset: call okenv_ddpg_create first")
    # after create, before set_params
    assert L.okenv_ddpg_create(h, C.byref(cfg)) == OK
    assert L.okenv_ddpg_num_params(h, None, None) == OK and L.okenv_ddpg_num_params(h, C.byref(a), C.byref(b)) == OK
    assert (a.value, b.value) == (3 * 8 + 8 + 8 * 2 + 2, 5 * 8 + 8 + 8 + 1)
    assert L.okenv_ddpg_set_params(h, None, None) == OK
    refused(small, h, L.okenv_ddpg_act(h, None), STATE, "okenv_ddpg_act: call okenv_ddpg_set_params first (the actor needs its parameters)")
    assert L.okenv_ddpg_set_params(h, None, capi.ptr(buf)) == OK  # the critic alone: acting still needs the actor, the state both
    small.sync()
    refused(small, h, L.okenv_ddpg_act(h, None), STATE, "okenv_ddpg_act: call okenv_ddpg_set_params first (the actor needs its parameters)")
    refused(small, h, L.okenv_ddpg_get_state(h, C.byref(st)), STATE,
            "okenv_ddpg_get_state: both networks need their parameters first (okenv_ddpg_create, okenv_ddpg_set_params)")
    assert L.okenv_ddpg_set_params(h, capi.ptr(buf), None) == OK
    small.sync()
    refused(small, h, L.okenv_ddpg_get_state(h, None), INVALID, "okenv_ddpg_get_state: NULL argument")
    assert L.okenv_ddpg_get_state(h, C.byref(st)) == OK and st.t == 0
    assert L.okenv_ddpg_set_draw_offset(h, None) == OK
    assert L.okenv_ddpg_act(h, None) == OK  # the gate opens
    small.sync()


def test_refusals_gauss(gpu, small):
    capi, L, h = gpu.capi, small._L, small._h
    cfg = capi.gauss_config(8, 8)
    n = C.c_int32(-1)
    st = capi.OkenvGaussState()
    buf = np.zeros(capi.gauss_num_params(3, 8, 8), dtype=f32)
    # a NULL handle
    refused(small, None, L.okenv_gauss_create(None, C.byref(cfg)), INVALID, "okenv_gauss_create: NULL handle")
    refused(small, None, L.okenv_gauss_create(None, None), INVALID, "okenv_gauss_create: NULL handle")
    refused(small, None, L.okenv_gauss_act(None, None), INVALID, "okenv_gauss_act: NULL handle")
    refused(small, None, L.okenv_gauss_num_params(None, C.byref(n)), STATE, "okenv_gauss_num_params: call okenv_gauss_create first")
    refused(small, None, L.okenv_gauss_set_params(None, capi.ptr(buf)), STATE, "okenv_gauss_set_params: call okenv_gauss_create first")
    refused(small, None, L.okenv_gauss_get_state(None, C.byref(st)), INVALID, "okenv_gauss_get_state: NULL argument")
    refused(small, None, L.okenv_gauss_get_params(None, None), INVALID, "okenv_gauss_get_params: NULL argument")
    refused(small, None, L.okenv_gauss_get_params(None, capi.ptr(buf)), INVALID, "okenv_gauss_get_state: NULL argument")
    refused(small, None, L.okenv_gauss_set_draw_offset(None, None), STATE, "okenv_gauss_set_draw_offset: call okenv_gauss_create first")
    refused(small, None, L.okenv_gauss_set_greedy(None, 1), STATE, "okenv_gauss_set_greedy: call okenv_gauss_create first")
    # before create: the state is checked before the argument
    refused(small, h, L.okenv_gauss_act(h, None), STATE, "okenv_gauss_act: call okenv_gauss_create first")
    refused(small, h, L.okenv_gauss_num_params(h, None), STATE, "okenv_gauss_num_params: call okenv_gauss_create first")
    refused(small, h, L.okenv_gauss_set_params(h, None), STATE, "okenv_gauss_set_params: call okenv_gauss_create first")
    refused(small, h, L.okenv_gauss_get_state(h, None), INVALID, "okenv_gauss_get_state: NULL argument")
    refused(small, h, L.okenv_gauss_get_state(h, C.byref(st)), STATE,
            "okenv_gauss_get_state: the actor needs its parameters first (okenv_gauss_create, okenv_gauss_set_params)")
    refused(small, h, L.okenv_gauss_get_params(h, None), INVALID, "okenv_gauss_get_params: NULL argument")
    refused(small, h, L.okenv_gauss_get_params(h, capi.ptr(buf)), STATE,
            "okenv_gauss_get_state: the actor needs its parameters first (okenv_gauss_create, okenv_gauss_set_params)")
    refused(small, h, L.okenv_gauss_set_draw_offset(h, None), STATE, "okenv_gauss_set_draw_offset: call okenv_gauss_create first")
    refused(small, h, L.okenv_gauss_set_greedy(h, 2), STATE, "okenv_gauss_set_greedy: call okenv_gauss_create first")
    # after create, before set_params
    assert L.okenv_gauss_create(h, C.byref(cfg)) == OK
    assert L.okenv_gauss_num_params(h, None) == OK and L.okenv_gauss_num_params(h, C.byref(n)) == OK and n.value == buf.size
    refused(small, h, L.okenv_gauss_set_params(h, None), INVALID, "okenv_gauss_set_params: NULL argument")
    refused(small, h, L.okenv_gauss_set_greedy(h, 2), INVALID, "okenv_gauss_set_greedy: greedy must be 0 or 1")
    refused(small, h, L.okenv_gauss_act(h, None), STATE, "okenv_gauss_act: call okenv_gauss_set_params first (the actor needs its parameters)")
    refused(small, h, L.okenv_gauss_get_state(h, C.byref(st)), STATE,
            "okenv_gauss_get_state: the actor needs its parameters first (okenv_gauss_create, okenv_gauss_set_params)")
    assert L.okenv_gauss_set_params(h, capi.ptr(buf)) == OK
    small.sync()
    assert L.okenv_gauss_get_state(h, C.byref(st)) == OK and st.t == 0
    assert L.okenv_gauss_set_greedy(h, 1) == OK and L.okenv_gauss_set_draw_offset(h, None) == OK
    assert L.okenv_gauss_act(h, None) == OK  # the gate opens
    small.sync()


def test_refusals_gcl(gpu, small):
    capi, L, h = gpu.capi, small._L, small._h
    cfg = capi.gcl_config(**GCL_WIDTHS)
    n = C.c_int32(-1)
    st = capi.OkenvGclState()
    buf = np.zeros(capi.gcl_num_params("policy", 3, 8, 8), dtype=f32)
    POLICY, COST = capi.GCL_NETWORKS["policy"], capi.GCL_NETWORKS["cost"]
    # a NULL handle
    refused(small, None, L.okenv_gcl_create(None, C.byref(cfg)), INVALID, "okenv_gcl_create: NULL handle")
    refused(small, None, L.okenv_gcl_create(None, None), INVALID, "okenv_gcl_create: NULL handle")
    refused(small, None, L.okenv_gcl_act(None, None), INVALID, "okenv_gcl_act: NULL handle")
    refused(small, None, L.okenv_gcl_num_params(None, POLICY, C.byref(n)), STATE, "okenv_gcl_num_params: call okenv_gcl_create first")
    refused(small, None, L.okenv_gcl_set_params(None, POLICY, capi.ptr(buf)), STATE, "okenv_gcl_set_params: call okenv_gcl_create first")
    refused(small, None, L.okenv_gcl_get_state(None, POLICY, C.byref(st)), INVALID, "okenv_gcl_get_state: NULL argument or unknown network")
    refused(small, None, L.okenv_gcl_get_params(None, POLICY, None), INVALID, "okenv_gcl_get_params: NULL argument")
    refused(small, None, L.okenv_gcl_get_params(None, POLICY, capi.ptr(buf)), INVALID, "okenv_gcl_get_state: NULL argument or unknown network")
    refused(small, None, L.okenv_gcl_set_draw_offset(None, None), STATE, "okenv_gcl_set_draw_offset: call okenv_gcl_create first")
    refused(small, None, L.okenv_gcl_set_greedy(None, 1), STATE, "okenv_gcl_set_greedy: call okenv_gcl_create first")
    # before create: the state is checked before the arguments
    refused(small, h, L.okenv_gcl_act(h, None), STATE, "okenv_gcl_act: call okenv_gcl_create first")
    refused(small, h, L.okenv_gcl_num_params(h, 7, None), STATE, "okenv_gcl_num_params: call okenv_gcl_create first")
    refused(small, h, L.okenv_gcl_set_params(h, 7, None), STATE, "okenv_gcl_set_params: call okenv_gcl_create first")
    refused(small, h, L.okenv_gcl_get_state(h, POLICY, None), INVALID, "okenv_gcl_get_state: NULL argument or unknown network")
    refused(small, h, L.okenv_gcl_get_state(h, 7, C.byref(st)), INVALID, "okenv_gcl_get_state: NULL argument or unknown network")
    refused(small, h, L.okenv_gcl_get_state(h, POLICY, C.byref(st)), STATE,
            "okenv_gcl_get_state: the network needs its parameters first (okenv_gcl_create, okenv_gcl_set_params)")
    refused(small, h, L.okenv_gcl_get_params(h, POLICY, None), INVALID, "okenv_gcl_get_params: NULL argument")
    refused(small, h, L.okenv_gcl_get_params(h, POLICY, capi.ptr(buf)), STATE,
            "okenv_gcl_get_state: the network needs its parameters first (okenv_gcl_create, okenv_gcl_set_params)")
    refused(small, h, L.okenv_gcl_set_draw_offset(h, None), STATE, "okenv_gcl_set_draw_offset: call okenv_gcl_create first")
    refused(small, h, L.okenv_gcl_set_greedy(h, 2), STATE, "okenv_gcl_set_greedy: call okenv_gcl_create first")
    # after create, before set_params
    assert L.okenv_gcl_create(h, C.byref(cfg)) == OK
    assert L.okenv_gcl_num_params(h, POLICY, None) == OK and L.okenv_gcl_num_params(h, POLICY, C.byref(n)) == OK and n.value == buf.size
    refused(small, h, L.okenv_gcl_num_params(h, 3, C.byref(n)), INVALID, "okenv_gcl_num_params: unknown network (OKENV_GCL_POLICY / _VALUE / _COST)")
    refused(small, h, L.okenv_gcl_num_params(h, -1, None), INVALID, "okenv_gcl_num_params: unknown network (OKENV_GCL_POLICY / _VALUE / _COST)")
    refused(small, h, L.okenv_gcl_set_params(h, POLICY, None), INVALID, "okenv_gcl_set_params: NULL argument or unknown network")
    refused(small, h, L.okenv_gcl_set_params(h, 3, capi.ptr(buf)), INVALID, "okenv_gcl_set_params: NULL argument or unknown network")
    refused(small, h, L.okenv_gcl_set_greedy(h, -1), INVALID, "okenv_gcl_set_greedy: greedy must be 0 or 1")
    refused(small, h, L.okenv_gcl_act(h, None), STATE, "okenv_gcl_act: call okenv_gcl_set_params first (the policy needs its parameters)")
    cost = np.zeros(capi.gcl_num_params("cost", 3, 8, 8), dtype=f32)
    assert L.okenv_gcl_set_params(h, COST, capi.ptr(cost)) == OK  # another network's parameters do not open the gate
    small.sync()
    refused(small, h, L.okenv_gcl_act(h, None), STATE, "okenv_gcl_act: call okenv_gcl_set_params first (the policy needs its parameters)")
    refused(small, h, L.okenv_gcl_get_state(h, POLICY, C.byref(st)), STATE,
            "okenv_gcl_get_state: the network needs its parameters first (okenv_gcl_create, okenv_gcl_set_params)")
    assert L.okenv_gcl_get_state(h, COST, C.byref(st)) == OK and st.t == 0
    assert L.okenv_gcl_set_params(h, POLICY, capi.ptr(buf)) == OK
    small.sync()
    assert L.okenv_gcl_get_state(h, POLICY, C.byref(st)) == OK and st.t == 0
    assert L.okenv_gcl_set_greedy(h, 0) == OK and L.okenv_gcl_set_draw_offset(h, None) == OK
    assert L.okenv_gcl_act(h, None) == OK  # the gate opens
    small.sync()


def test_refusals_lidar(gpu, small):
    capi, L, h = gpu.capi, small._L, small._h
    cfg = capi.lidar_config(**lidar_mirror.SHAPES["tiny"])
    n = C.c_int32(-1)
    buf = np.zeros(capi.lidar_num_params(cfg), dtype=f32)
    # a NULL handle, a NULL pointer: the argument is checked before the state
    refused(small, None, L.okenv_lidar_create(None, C.byref(cfg)), INVALID, "okenv_lidar_create: NULL handle")
    refused(small, None, L.okenv_lidar_create(None, None), INVALID, "okenv_lidar_create: NULL handle")
    refused(small, None, L.okenv_lidar_act(None, None), INVALID, "okenv_lidar_act: NULL handle")
    refused(small, None, L.okenv_lidar_num_params(None, C.byref(n)), INVALID, "okenv_lidar_num_params: NULL argument")
    refused(small, None, L.okenv_lidar_set_params(None, capi.ptr(buf)), INVALID, "okenv_lidar_set_params: NULL argument")
    refused(small, None, L.okenv_lidar_get_params(None, capi.ptr(buf)), INVALID, "okenv_lidar_get_params: NULL argument")
    # before create
    refused(small, h, L.okenv_lidar_act(h, None), STATE, "okenv_lidar_act: call okenv_lidar_create first")
    refused(small, h, L.okenv_lidar_num_params(h, None), INVALID, "okenv_lidar_num_params: NULL argument")
    refused(small, h, L.okenv_lidar_num_params(h, C.byref(n)), STATE, "okenv_lidar_num_params: call okenv_lidar_create first")
    refused(small, h, L.okenv_lidar_set_params(h, None), INVALID, "okenv_lidar_set_params: NULL argument")
    refused(small, h, L.okenv_lidar_set_params(h, capi.ptr(buf)), STATE, "okenv_lidar_set_params: call okenv_lidar_create first")
    refused(small, h, L.okenv_lidar_get_params(h, None), INVALID, "okenv_lidar_get_params: NULL argument")
    refused(small, h, L.okenv_lidar_get_params(h, capi.ptr(buf)), STATE,
            "okenv_lidar_get_params: the policy needs its parameters first (okenv_lidar_create, okenv_lidar_set_params)")
    assert n.value == -1
    # after create, before set_params
    assert L.okenv_lidar_create(h, C.byref(cfg)) == OK
    refused(small, h, L.okenv_lidar_num_params(h, None), INVALID, "okenv_lidar_num_params: NULL argument")
    assert L.okenv_lidar_num_params(h, C.byref(n)) == OK and n.value == buf.size
    refused(small, h, L.okenv_lidar_set_params(h, None), INVALID, "okenv_lidar_set_params: NULL argument")
    refused(small, h, L.okenv_lidar_act(h, None), STATE, "okenv_lidar_act: call okenv_lidar_set_params first (the policy needs its parameters)")
    refused(small, h, L.okenv_lidar_get_params(h, capi.ptr(buf)), STATE,
            "okenv_lidar_get_params: the policy needs its parameters first (okenv_lidar_create, okenv_lidar_set_params)")
    assert L.okenv_lidar_set_params(h, capi.ptr(buf)) == OK
    small.sync()
    refused(small, h, L.okenv_lidar_get_params(h, None), INVALID, "okenv_lidar_get_params: NULL argument")
    assert L.okenv_lidar_get_params(h, capi.ptr(buf)) == OK
    assert L.okenv_lidar_act(h, None) == OK  # the gate opens
    small.sync()


def test_refusals_flow(gpu, small):
    capi, L, h = gpu.capi, small._L, small._h
    cfg = capi.flow_config(**flow_mirror.SHAPES["tiny"])
    n = C.c_int32(-1)
    buf = np.zeros(capi.flow_num_params(cfg), dtype=f32)
    cond = torch.zeros((3, cfg.cond_dim), device="cuda")
    torch.cuda.synchronize()
    # a NULL handle, a NULL pointer: the argument is checked before the state
    refused(small, None, L.okenv_flow_create(None, C.byref(cfg)), INVALID, "okenv_flow_create: NULL handle")
    refused(small, None, L.okenv_flow_create(None, None), INVALID, "okenv_flow_create: NULL handle")
    refused(small, None, L.okenv_flow_act(None, capi.ptr(cond), None), INVALID, "okenv_flow_act: NULL handle")
    refused(small, None, L.okenv_flow_num_params(None, C.byref(n)), INVALID, "okenv_flow_num_params: NULL argument")
    refused(small, None, L.okenv_flow_set_params(None, capi.ptr(buf)), INVALID, "okenv_flow_set_params: NULL argument")
    refused(small, None, L.okenv_flow_get_params(None, capi.ptr(buf)), INVALID, "okenv_flow_get_params: NULL argument")
    refused(small, None, L.okenv_flow_set_draw_offset(None, None), STATE, "okenv_flow_set_draw_offset: call okenv_flow_create first")
    # before create (a NULL cond comes behind the state)
    refused(small, h, L.okenv_flow_act(h, capi.ptr(cond), None), STATE, "okenv_flow_act: call okenv_flow_create first")
    refused(small, h, L.okenv_flow_act(h, None, None), STATE, "okenv_flow_act: call okenv_flow_create first")
    refused(small, h, L.okenv_flow_num_params(h, None), INVALID, "okenv_flow_num_params: NULL argument")
    refused(small, h, L.okenv_flow_num_params(h, C.byref(n)), STATE, "okenv_flow_num_params: call okenv_flow_create first")
    refused(small, h, L.okenv_flow_set_params(h, None), INVALID, "okenv_flow_set_params: NULL argument")
    refused(small, h, L.okenv_flow_set_params(h, capi.ptr(buf)), STATE, "okenv_flow_set_params: call okenv_flow_create first")
    refused(small, h, L.okenv_flow_get_params(h, None), INVALID, "okenv_flow_get_params: NULL argument")
    refused(small, h, L.okenv_flow_get_params(h, capi.ptr(buf)), STATE,
            "okenv_flow_get_params: the policy needs its parameters first (okenv_flow_create, okenv_flow_set_params)")
    refused(small, h, L.okenv_flow_set_draw_offset(h, None), STATE, "okenv_flow_set_draw_offset: call okenv_flow_create first")
    assert n.value == -1
    # after create, before set_params
    assert L.okenv_flow_create(h, C.byref(cfg)) == OK
    refused(small, h, L.okenv_flow_num_params(h, None), INVALID, "okenv_flow_num_params: NULL argument")
    assert L.okenv_flow_num_params(h, C.byref(n)) == OK and n.value == buf.size
    refused(small, h, L.okenv_flow_set_params(h, None), INVALID, "okenv_flow_set_params: NULL argument")
    refused(small, h, L.okenv_flow_act(h, capi.ptr(cond), None), STATE, "okenv_flow_act: call okenv_flow_set_params first (the policy needs its parameters)")
    refused(small, h, L.okenv_flow_act(h, None, None), STATE, "okenv_flow_act: call okenv_flow_set_params first (the policy needs its parameters)")
    refused(small, h, L.okenv_flow_get_params(h, capi.ptr(buf)), STATE,
            "okenv_flow_get_params: the policy needs its parameters first (okenv_flow_create, okenv_flow_set_params)")
    assert L.okenv_flow_set_params(h, capi.ptr(buf)) == OK
    small.sync()
    refused(small, h, L.okenv_flow_act(h, None, None), INVALID, "okenv_flow_act: cond is NULL")
    assert L.okenv_flow_get_params(h, capi.ptr(buf)) == OK and L.okenv_flow_set_draw_offset(h, None) == OK
    assert L.okenv_flow_act(h, capi.ptr(cond), None) == OK  # the gate opens
    small.sync()


# The image families with one vector (bev, cnn, qcnn, vit) share the order of their checks; `entry` is "act" or "encode", `who` the
# subject of "needs its parameters", act(handle, frames, frame_bytes) the raw call with the test's own record or output.
FRAME_BYTES = "frame_bytes is not num_agents x image_size x image_size x 4"


def random_frames(N, S, seed):
    torch.manual_seed(seed)
    frames = torch.randint(0, 256, (N, S, S, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # the handle has a stream of its own
    return frames


def ptr(a):
    from openkitchen_amd import capi
    return capi.ptr(a)


def params_entries(dev, prefix):
    return [getattr(dev._L, prefix + e) for e in ("num_params", "set_params", "get_params")]


def image_before_create(dev, h, prefix, who, entry, cfg, params, act, frames):
    """A NULL handle, a NULL pointer and the state before create: num_params, set_params and get_params look at their pointer before
    the state (kGateArgFirst); create and act name the NULL handle; act looks at the state before its frames."""
    create = getattr(dev._L, prefix + "create")
    num, set_, get = params_entries(dev, prefix)
    n, buf = C.c_int32(-1), np.zeros_like(params)
    needs = "%sget_params: %s needs its parameters first (%screate, %sset_params)" % (prefix, who, prefix, prefix)
    refused(dev, None, create(None, C.byref(cfg)), INVALID, prefix + "create: NULL handle")
    refused(dev, None, create(None, None), INVALID, prefix + "create: NULL handle")
    refused(dev, None, act(None, frames, frames.numel()), INVALID, prefix + entry + ": NULL handle")
    for handle in (None, h):
        refused(dev, handle, num(handle, None), INVALID, prefix + "num_params: NULL argument")
        refused(dev, handle, set_(handle, None), INVALID, prefix + "set_params: NULL argument")
        refused(dev, handle, get(handle, None), INVALID, prefix + "get_params: NULL argument")
    refused(dev, None, num(None, C.byref(n)), INVALID, prefix + "num_params: NULL argument")
    refused(dev, None, set_(None, ptr(params)), INVALID, prefix + "set_params: NULL argument")
    refused(dev, None, get(None, ptr(buf)), INVALID, prefix + "get_params: NULL argument")
    refused(dev, h, num(h, C.byref(n)), STATE, prefix + "num_params: call " + prefix + "create first")
    refused(dev, h, set_(h, ptr(params)), STATE, prefix + "set_params: call " + prefix + "create first")
    refused(dev, h, get(h, ptr(buf)), STATE, needs)
    refused(dev, h, act(h, frames, frames.numel()), STATE, prefix + entry + ": call " + prefix + "create first")
    refused(dev, h, act(h, None, 0), STATE, prefix + entry + ": call " + prefix + "create first")
    refused(dev, h, create(h, None), INVALID, prefix + "create: config is NULL")
    refused(dev, h, act(h, frames, frames.numel()), STATE, prefix + entry + ": call " + prefix + "create first")
    assert n.value == -1


def image_created(dev, h, prefix, who, entry, cfg, params, act, frames):
    """After create, before set_params: the count is there, the vector and the act are not (the frames are not looked at yet)."""
    create = getattr(dev._L, prefix + "create")
    num, set_, get = params_entries(dev, prefix)
    n, buf = C.c_int32(-1), np.zeros_like(params)
    assert create(h, C.byref(cfg)) == OK
    refused(dev, h, num(h, None), INVALID, prefix + "num_params: NULL argument")
    assert num(h, C.byref(n)) == OK and n.value == params.size
    refused(dev, h, set_(h, None), INVALID, prefix + "set_params: NULL argument")
    refused(dev, h, get(h, ptr(buf)), STATE, "%sget_params: %s needs its parameters first (%screate, %sset_params)" % (prefix, who, prefix, prefix))
    for args in ((frames, frames.numel()), (None, frames.numel()), (frames, 0)):
        refused(dev, h, act(h, *args), STATE, "%s%s: call %sset_params first (%s needs its parameters)" % (prefix, entry, prefix, who))


def image_gate_opens(dev, h, prefix, entry, cfg, params, act, frames, result, bad_frames, bad_configs):
    """With parameters: they come back bit for bit; a bad frames argument is refused in the entry's words (bad_frames: ((frames,
    frame_bytes), text)); the gate opens; a create refused for its config (bad_configs: (config or None, text)) leaves the driver
    attached, parameterised and acting as before.  result(): what the act wrote, as numpy arrays."""
    create = getattr(dev._L, prefix + "create")
    num, set_, get = params_entries(dev, prefix)
    buf = np.zeros_like(params)
    assert set_(h, ptr(params)) == OK
    dev.sync()
    refused(dev, h, get(h, None), INVALID, prefix + "get_params: NULL argument")
    assert get(h, ptr(buf)) == OK and same(buf, params)
    for args, text in (((None, frames.numel()), "NULL argument"), ((frames, frames.numel() - 4), FRAME_BYTES), ((frames, 0), FRAME_BYTES)) + tuple(bad_frames):
        refused(dev, h, act(h, *args), INVALID, prefix + entry + ": " + text)
    assert act(h, frames, frames.numel()) == OK  # the gate opens
    before = result()
    for bad, text in ((None, "config is NULL"),) + tuple(bad_configs):
        refused(dev, h, create(h, None if bad is None else C.byref(bad)), INVALID, prefix + "create: " + text)
    buf[:] = 0
    assert get(h, ptr(buf)) == OK and same(buf, params)
    assert act(h, frames, frames.numel()) == OK
    after = result()
    assert all(same(a, b) for a, b in zip(before, after)) and any(np.any(b) for b in before)


def test_refusals_bev(gpu, small):
    capi, L, h = gpu.capi, small._L, small._h
    shape = bev_mirror.SHAPES["tiny"]
    cfg, params = capi.bev_config(**shape), bev_mirror.draw_params(shape, 1)
    frames = random_frames(3, shape["image_size"], 51)
    out = torch.zeros((3, shape["embed_dim"]), device="cuda")
    torch.cuda.synchronize()

    def encode(handle, f, nbytes):
        return L.okenv_bev_encode(handle, capi.ptr(f), nbytes, capi.ptr(out))

    def result():
        small.sync()
        got = out.cpu().numpy()
        out.zero_()
        torch.cuda.synchronize()
        return (got,)

    family = (small, h, "okenv_bev_", "the encoder", "encode", cfg, params, encode, frames)
    image_before_create(*family)
    image_created(*family)
    limits = ("shape outside the limits (image_size a multiple of 8 in 16 .. 128; kernel 3 or 5; channels multiples of 16 in 16 .. 128; "
              "embed_dim a multiple of 16 in 16 .. 512)")
    image_gate_opens(small, h, "okenv_bev_", "encode", cfg, params, encode, frames, result, (), ((capi.bev_config(**dict(shape, image_size=12)), limits),))
    refused(small, h, L.okenv_bev_encode(h, capi.ptr(frames), frames.numel(), None), INVALID, "okenv_bev_encode: NULL argument")  # the output


def test_refusals_cnn(gpu, small):
    capi, L, h = gpu.capi, small._L, small._h
    shape = cnn_mirror.SHAPES["tiny"]
    cfg, params = capi.cnn_config(**shape), cnn_mirror.draw_params(shape, 1)
    frames = random_frames(3, shape["image_size"], 52)
    rec = {"out": torch.zeros(3, device="cuda"), "action": torch.zeros((3, 2), device="cuda"), "alive": torch.zeros(3, dtype=torch.uint8, device="cuda")}
    torch.cuda.synchronize()
    struct = capi.fill_pointers(capi.OkenvCnnRecord(), rec, "record")

    def act(handle, f, nbytes):
        return L.okenv_cnn_act(handle, capi.ptr(f), nbytes, C.byref(struct))

    def result():
        small.sync()
        got = tuple(t.cpu().numpy() for t in rec.values())
        for t in rec.values():
            t.zero_()
        torch.cuda.synchronize()
        return got

    family = (small, h, "okenv_cnn_", "the policy", "act", cfg, params, act, frames)
    image_before_create(*family)
    image_created(*family)
    image_gate_opens(small, h, "okenv_cnn_", "act", cfg, params, act, frames, result,
                     (((frames.data_ptr() + 1, frames.numel()), "frames must be 4-byte aligned"),),
                     ((capi.cnn_config(**dict(shape, steer_scale=float("nan"))), "throttle / steer_scale must be finite"),))


def test_refusals_qcnn(gpu, small):
    capi, L, h = gpu.capi, small._L, small._h
    shape = qcnn_mirror.SHAPES["tiny"]
    cfg, params = qcnn_config(capi, "tiny"), qcnn_mirror.draw_params(shape, 1)
    frames = random_frames(3, shape["image_size"], 53)
    rec = {"q": torch.zeros((3, shape["num_actions"]), device="cuda"), "action": torch.zeros(3, dtype=torch.int64, device="cuda"),
           "value": torch.zeros(3, device="cuda"), "alive": torch.zeros(3, dtype=torch.uint8, device="cuda")}
    torch.cuda.synchronize()
    struct = capi.fill_pointers(capi.OkenvQcnnRecord(), rec, "record")

    def act(handle, f, nbytes):
        return L.okenv_qcnn_act(handle, capi.ptr(f), nbytes, C.byref(struct))

    def result():
        small.sync()
        got = tuple(t.cpu().numpy() for t in rec.values())
        for t in rec.values():
            t.zero_()
        torch.cuda.synchronize()
        return got

    family = (small, h, "okenv_qcnn_", "the network", "act", cfg, params, act, frames)
    for handle in (None, h):  # the two setters: the state only
        refused(small, handle, L.okenv_qcnn_set_draw_offset(handle, None), STATE, "okenv_qcnn_set_draw_offset: call okenv_qcnn_create first")
        refused(small, handle, L.okenv_qcnn_set_epsilon(handle, 0.5), STATE, "okenv_qcnn_set_epsilon: call okenv_qcnn_create first")
        refused(small, handle, L.okenv_qcnn_set_epsilon(handle, 1.5), STATE, "okenv_qcnn_set_epsilon: call okenv_qcnn_create first")
    image_before_create(*family)
    image_created(*family)
    refused(small, h, L.okenv_qcnn_set_epsilon(h, 1.5), INVALID, "okenv_qcnn_set_epsilon: epsilon outside [0, 1]")
    refused(small, h, L.okenv_qcnn_set_epsilon(h, float("nan")), INVALID, "okenv_qcnn_set_epsilon: epsilon outside [0, 1]")
    assert L.okenv_qcnn_set_epsilon(h, 0.0) == OK and L.okenv_qcnn_set_draw_offset(h, None) == OK
    aligned = "frames must be 16-byte aligned (4-byte where image_size x image_size is no multiple of 4)"
    image_gate_opens(small, h, "okenv_qcnn_", "act", cfg, params, act, frames, result, (((frames.data_ptr() + 4, frames.numel()), aligned),),
                     ((qcnn_config(capi, "tiny", "eps_greedy", 1.5), "epsilon outside [0, 1]"), (qcnn_config(capi, "tiny", "sample"), "unknown mode (OKENV_ACTOR_GREEDY / _EPS_GREEDY)")))


def test_refusals_vit(gpu, small):
    capi, L, h = gpu.capi, small._L, small._h
    shape = vit_mirror.SHAPES["tiny"]
    cfg = capi.vit_config(**shape)
    params = vit_mirror.random_params(capi, cfg, np.random.default_rng(54), scale=2.0)
    S, D = shape["image_size"], shape["dim"]
    frames = random_frames(3, S, 54)
    rec = {"action": torch.zeros((3, 2), device="cuda"), "output": torch.zeros(3, device="cuda"), "embedding": torch.zeros((3, D), device="cuda"),
           "alive": torch.zeros(3, dtype=torch.uint8, device="cuda")}
    embedding = torch.zeros((2, D), device="cuda")
    torch.cuda.synchronize()
    struct = capi.fill_pointers(capi.OkenvVitRecord(), rec, "record")

    def act(handle, f, nbytes):
        return L.okenv_vit_act(handle, capi.ptr(f), nbytes, C.byref(struct))

    def embed(handle, f=frames, m=2, nbytes=2 * S * S * 4, out=embedding):
        return L.okenv_vit_embed(handle, capi.ptr(f), m, nbytes, capi.ptr(out))

    def result():
        small.sync()
        got = tuple(t.cpu().numpy() for t in rec.values())
        for t in rec.values():
            t.zero_()
        torch.cuda.synchronize()
        return got

    family = (small, h, "okenv_vit_", "the policy", "act", cfg, params, act, frames)
    refused(small, None, embed(None), INVALID, "okenv_vit_embed: NULL handle")
    refused(small, h, embed(h), STATE, "okenv_vit_embed: call okenv_vit_create first")
    refused(small, h, embed(h, None, 0, 0, None), STATE, "okenv_vit_embed: call okenv_vit_create first")
    image_before_create(*family)
    image_created(*family)
    refused(small, h, embed(h), STATE, "okenv_vit_embed: call okenv_vit_set_params first (the policy needs its parameters)")
    refused(small, h, embed(h, None, 0, 0, None), STATE, "okenv_vit_embed: call okenv_vit_set_params first (the policy needs its parameters)")
    image_gate_opens(small, h, "okenv_vit_", "act", cfg, params, act, frames, result, (((frames.data_ptr() + 1, frames.numel()), "frames must be 4-byte aligned"),),
                     ((capi.vit_config(**dict(shape, ln_eps=0.0)), "ln_eps must be finite and > 0"),
                      (capi.vit_config(**dict(shape, agents_per_pass=-1)), "agents_per_pass and workspace_bytes must not be negative")))
    # okenv_vit_embed counts its frames by m, not by the population, and says so in a text of its own
    own = "okenv_vit_embed: m must be at least 1 and frame_bytes m x image_size x image_size x 4"
    refused(small, h, embed(h, None), INVALID, "okenv_vit_embed: NULL argument")
    refused(small, h, embed(h, out=None), INVALID, "okenv_vit_embed: NULL argument")
    refused(small, h, embed(h, m=0, nbytes=0), INVALID, own)
    refused(small, h, embed(h, m=3), INVALID, own)
    refused(small, h, embed(h, nbytes=2 * S * S * 4 - 4), INVALID, own)
    refused(small, h, embed(h, frames.data_ptr() + 1), INVALID, "okenv_vit_embed: frames must be 4-byte aligned")
    assert embed(h) == OK
    small.sync()
    assert same(embedding.cpu().numpy(), capi.vit_act_host(cfg, params, frames.cpu().numpy()[:2])["embedding"])


def test_refusals_world(gpu, small):
    capi, L, h = gpu.capi, small._L, small._h
    shape = world_mirror.SHAPES["tiny"]
    cfg = capi.world_config(**shape)
    enc, ctrl = world_mirror.draw_params(shape, 1, 3)
    frames = random_frames(3, shape["image_size"], 55)
    nbytes = frames.numel()
    a, b = C.c_int32(-1), C.c_int32(-1)
    buf, cbuf = np.zeros_like(enc), np.zeros_like(ctrl)
    ENCODER, CONTROLLERS = capi.WORLD_ENCODER, capi.WORLD_VECTORS["controllers"]
    which = "which must be OKENV_WORLD_ENCODER or OKENV_WORLD_CONTROLLERS"
    stored = "okenv_world_get_params: the vector needs its parameters first (okenv_world_create, okenv_world_set_params)"
    unset = "okenv_world_act: call okenv_world_set_params first (the encoder and the controllers need their parameters)"

    def act(handle, f=frames, n=nbytes):
        return L.okenv_world_act(handle, capi.ptr(f), n, None)

    # a NULL handle, a NULL pointer: the argument is checked before the state, and before `which`
    refused(small, None, L.okenv_world_create(None, C.byref(cfg)), INVALID, "okenv_world_create: NULL handle")
    refused(small, None, L.okenv_world_create(None, None), INVALID, "okenv_world_create: NULL handle")
    refused(small, None, act(None), INVALID, "okenv_world_act: NULL handle")
    refused(small, None, L.okenv_world_num_params(None, C.byref(a), C.byref(b)), INVALID, "okenv_world_num_params: NULL argument")
    refused(small, None, L.okenv_world_set_params(None, ENCODER, capi.ptr(enc)), INVALID, "okenv_world_set_params: NULL argument")
    refused(small, None, L.okenv_world_get_params(None, ENCODER, capi.ptr(buf)), INVALID, "okenv_world_get_params: NULL argument")
    # before create
    refused(small, h, act(h), STATE, "okenv_world_act: call okenv_world_create first")
    refused(small, h, act(h, None, 0), STATE, "okenv_world_act: call okenv_world_create first")
    refused(small, h, L.okenv_world_num_params(h, None, C.byref(b)), INVALID, "okenv_world_num_params: NULL argument")
    refused(small, h, L.okenv_world_num_params(h, C.byref(a), None), INVALID, "okenv_world_num_params: NULL argument")
    refused(small, h, L.okenv_world_num_params(h, C.byref(a), C.byref(b)), STATE, "okenv_world_num_params: call okenv_world_create first")
    refused(small, h, L.okenv_world_set_params(h, 7, None), INVALID, "okenv_world_set_params: NULL argument")
    refused(small, h, L.okenv_world_set_params(h, ENCODER, capi.ptr(enc)), STATE, "okenv_world_set_params: call okenv_world_create first")
    refused(small, h, L.okenv_world_set_params(h, 7, capi.ptr(enc)), STATE, "okenv_world_set_params: call okenv_world_create first")  # `which` comes behind
    refused(small, h, L.okenv_world_get_params(h, 7, None), INVALID, "okenv_world_get_params: NULL argument")
    for w in (ENCODER, CONTROLLERS, 7):
        refused(small, h, L.okenv_world_get_params(h, w, capi.ptr(cbuf)), STATE, stored)
    refused(small, h, L.okenv_world_create(h, None), INVALID, "okenv_world_create: config is NULL")
    assert (a.value, b.value) == (-1, -1)
    # after create, before set_params
    assert L.okenv_world_create(h, C.byref(cfg)) == OK
    refused(small, h, L.okenv_world_num_params(h, None, None), INVALID, "okenv_world_num_params: NULL argument")
    assert L.okenv_world_num_params(h, C.byref(a), C.byref(b)) == OK and (a.value, b.value) == (enc.size, ctrl.shape[1])
    refused(small, h, L.okenv_world_set_params(h, 7, None), INVALID, "okenv_world_set_params: NULL argument")
    refused(small, h, L.okenv_world_set_params(h, 7, capi.ptr(enc)), INVALID, "okenv_world_set_params: " + which)
    refused(small, h, L.okenv_world_set_params(h, -1, capi.ptr(enc)), INVALID, "okenv_world_set_params: " + which)
    for w in (ENCODER, CONTROLLERS, 7):  # get_params refuses through the gate before it looks at `which`
        refused(small, h, L.okenv_world_get_params(h, w, capi.ptr(cbuf)), STATE, stored)
    refused(small, h, act(h), STATE, unset)
    refused(small, h, act(h, None, 0), STATE, unset)
    assert L.okenv_world_set_params(h, ENCODER, capi.ptr(enc)) == OK
    small.sync()
    refused(small, h, act(h), STATE, unset)  # the controllers are still missing
    refused(small, h, L.okenv_world_get_params(h, CONTROLLERS, capi.ptr(cbuf)), STATE, stored)
    refused(small, h, L.okenv_world_get_params(h, 7, capi.ptr(cbuf)), INVALID, "okenv_world_get_params: " + which)  # (not the controllers: flag 1 is asked)
    assert L.okenv_world_get_params(h, ENCODER, capi.ptr(buf)) == OK and same(buf, enc)
    assert L.okenv_world_set_params(h, CONTROLLERS, capi.ptr(ctrl)) == OK
    small.sync()
    assert L.okenv_world_get_params(h, CONTROLLERS, capi.ptr(cbuf)) == OK and same(cbuf, ctrl)
    # with both vectors: the frames are looked at, the gate opens
    refused(small, h, act(h, None), INVALID, "okenv_world_act: NULL argument")
    refused(small, h, act(h, frames, nbytes - 4), INVALID, "okenv_world_act: " + FRAME_BYTES)
    refused(small, h, act(h, frames.data_ptr() + 1), INVALID, "okenv_world_act: frames must be 4-byte aligned")
    assert act(h) == OK
    small.sync()
    before = small.get(capi.F_STEER)
    # a create refused for its config leaves the racers attached, parameterised and acting as before
    refused(small, h, L.okenv_world_create(h, None), INVALID, "okenv_world_create: config is NULL")
    refused(small, h, L.okenv_world_create(h, C.byref(capi.world_config(**dict(shape, skip_crashed=2)))), INVALID, "okenv_world_create: skip_crashed must be 0 or 1")
    small.set(capi.F_STEER, np.full(3, -3.0, f32))
    assert act(h) == OK
    small.sync()
    assert same(small.get(capi.F_STEER), before) and same(before, world_host_act(capi, cfg, enc, ctrl, frames, small)["steer"])


def test_refusals_memory(gpu):
    """On a handle of its own: the memory stands on the racers, and what it says while they are missing comes first."""
    capi = gpu.capi
    dev = population(gpu, 3, 3)
    L, h = dev._L, dev._h
    wc, mc = memory_configs(capi, "h16")
    enc, net, ctrl, hidden = memory_drawn("h16", 1, 3)
    frames = random_frames(3, wc.image_size, 56)
    nbytes = frames.numel()
    a, b = C.c_int32(-1), C.c_int32(-1)
    buf, cbuf, hbuf = np.zeros_like(net), np.zeros_like(ctrl), np.zeros_like(hidden)
    NETWORK, CONTROLLERS = capi.MEMORY_NETWORK, capi.MEMORY_VECTORS["controllers"]
    which = "which must be OKENV_MEMORY_NETWORK or OKENV_MEMORY_CONTROLLERS"
    first = "call okenv_memory_create first"
    stored = "okenv_memory_get_params: the vector needs its parameters first (okenv_memory_create, okenv_memory_set_params)"
    unset = "okenv_memory_act: call okenv_memory_set_params first (the network and the controllers need their parameters)"

    def act(handle, f=frames, n=nbytes):
        return L.okenv_memory_act(handle, capi.ptr(f), n, None)

    # a NULL handle, a NULL pointer: the argument is checked before the state, and before `which`
    refused(dev, None, L.okenv_memory_create(None, C.byref(mc)), INVALID, "okenv_memory_create: NULL handle")
    refused(dev, None, L.okenv_memory_create(None, None), INVALID, "okenv_memory_create: NULL handle")
    refused(dev, None, act(None), INVALID, "okenv_memory_act: NULL handle")
    refused(dev, None, L.okenv_memory_reset(None), INVALID, "okenv_memory_reset: NULL handle")
    refused(dev, None, L.okenv_memory_num_params(None, C.byref(a), C.byref(b)), INVALID, "okenv_memory_num_params: NULL argument")
    refused(dev, None, L.okenv_memory_set_params(None, NETWORK, capi.ptr(net)), INVALID, "okenv_memory_set_params: NULL argument")
    refused(dev, None, L.okenv_memory_get_params(None, NETWORK, capi.ptr(buf)), INVALID, "okenv_memory_get_params: NULL argument")
    refused(dev, None, L.okenv_memory_set_hidden(None, capi.ptr(hidden)), INVALID, "okenv_memory_set_hidden: NULL argument")
    refused(dev, None, L.okenv_memory_get_hidden(None, capi.ptr(hbuf)), INVALID, "okenv_memory_get_hidden: NULL argument")
    # before okenv_world_create: create says so before it looks at its config
    refused(dev, h, L.okenv_memory_create(h, C.byref(mc)), STATE, "okenv_memory_create: call okenv_world_create first")
    refused(dev, h, L.okenv_memory_create(h, None), STATE, "okenv_memory_create: call okenv_world_create first")
    refused(dev, h, act(h), STATE, "okenv_memory_act: " + first)
    assert L.okenv_world_create(h, C.byref(wc)) == OK
    # before okenv_memory_create
    refused(dev, h, L.okenv_memory_create(h, None), INVALID, "okenv_memory_create: config is NULL")
    refused(dev, h, act(h), STATE, "okenv_memory_act: " + first)
    refused(dev, h, act(h, None, 0), STATE, "okenv_memory_act: " + first)
    refused(dev, h, L.okenv_memory_reset(h), STATE, "okenv_memory_reset: " + first)
    refused(dev, h, L.okenv_memory_num_params(h, None, C.byref(b)), INVALID, "okenv_memory_num_params: NULL argument")
    refused(dev, h, L.okenv_memory_num_params(h, C.byref(a), None), INVALID, "okenv_memory_num_params: NULL argument")
    refused(dev, h, L.okenv_memory_num_params(h, C.byref(a), C.byref(b)), STATE, "okenv_memory_num_params: " + first)
    refused(dev, h, L.okenv_memory_set_params(h, 7, None), INVALID, "okenv_memory_set_params: NULL argument")
    refused(dev, h, L.okenv_memory_set_params(h, NETWORK, capi.ptr(net)), STATE, "okenv_memory_set_params: " + first)
    refused(dev, h, L.okenv_memory_set_params(h, 7, capi.ptr(net)), STATE, "okenv_memory_set_params: " + first)  # `which` comes behind
    refused(dev, h, L.okenv_memory_get_params(h, 7, None), INVALID, "okenv_memory_get_params: NULL argument")
    for w in (NETWORK, CONTROLLERS, 7):
        refused(dev, h, L.okenv_memory_get_params(h, w, capi.ptr(cbuf)), STATE, stored)
    refused(dev, h, L.okenv_memory_set_hidden(h, None), INVALID, "okenv_memory_set_hidden: NULL argument")
    refused(dev, h, L.okenv_memory_set_hidden(h, capi.ptr(hidden)), STATE, "okenv_memory_set_hidden: " + first)
    refused(dev, h, L.okenv_memory_get_hidden(h, None), INVALID, "okenv_memory_get_hidden: NULL argument")
    refused(dev, h, L.okenv_memory_get_hidden(h, capi.ptr(hbuf)), STATE, "okenv_memory_get_hidden: " + first)
    assert (a.value, b.value) == (-1, -1)
    # after create, before any set_params: the racers' encoder is asked for before the memory's own vectors and before the frames
    assert L.okenv_memory_create(h, C.byref(mc)) == OK
    refused(dev, h, L.okenv_memory_num_params(h, None, None), INVALID, "okenv_memory_num_params: NULL argument")
    assert L.okenv_memory_num_params(h, C.byref(a), C.byref(b)) == OK and (a.value, b.value) == (net.size, ctrl.shape[1])
    for args in ((frames, nbytes), (None, 0)):
        refused(dev, h, act(h, *args), STATE, "okenv_memory_act: call okenv_world_set_params first (the encoder needs its parameters)")
    assert L.okenv_world_set_params(h, capi.WORLD_ENCODER, capi.ptr(enc)) == OK
    dev.sync()
    refused(dev, h, act(h), STATE, unset)
    refused(dev, h, act(h, None, 0), STATE, unset)
    refused(dev, h, L.okenv_memory_set_params(h, 7, None), INVALID, "okenv_memory_set_params: NULL argument")
    refused(dev, h, L.okenv_memory_set_params(h, 7, capi.ptr(net)), INVALID, "okenv_memory_set_params: " + which)
    for w in (NETWORK, CONTROLLERS, 7):  # get_params refuses through the gate before it looks at `which`
        refused(dev, h, L.okenv_memory_get_params(h, w, capi.ptr(cbuf)), STATE, stored)
    assert L.okenv_memory_set_params(h, NETWORK, capi.ptr(net)) == OK
    dev.sync()
    refused(dev, h, act(h), STATE, unset)  # the controllers are still missing
    refused(dev, h, L.okenv_memory_get_params(h, CONTROLLERS, capi.ptr(cbuf)), STATE, stored)
    refused(dev, h, L.okenv_memory_get_params(h, 7, capi.ptr(cbuf)), INVALID, "okenv_memory_get_params: " + which)
    assert L.okenv_memory_get_params(h, NETWORK, capi.ptr(buf)) == OK and same(buf, net)
    assert L.okenv_memory_set_params(h, CONTROLLERS, capi.ptr(ctrl)) == OK
    dev.sync()
    assert L.okenv_memory_get_params(h, CONTROLLERS, capi.ptr(cbuf)) == OK and same(cbuf, ctrl)
    # the hidden state's entries need the create only
    refused(dev, h, L.okenv_memory_set_hidden(h, None), INVALID, "okenv_memory_set_hidden: NULL argument")
    refused(dev, h, L.okenv_memory_get_hidden(h, None), INVALID, "okenv_memory_get_hidden: NULL argument")
    assert L.okenv_memory_set_hidden(h, capi.ptr(hidden)) == OK
    dev.sync()
    assert L.okenv_memory_get_hidden(h, capi.ptr(hbuf)) == OK and same(hbuf, hidden)
    assert L.okenv_memory_reset(h) == OK and L.okenv_memory_get_hidden(h, capi.ptr(hbuf)) == OK and not hbuf.any()
    # with every vector: the frames are looked at, the gate opens
    refused(dev, h, act(h, None), INVALID, "okenv_memory_act: NULL argument")
    refused(dev, h, act(h, frames, nbytes - 4), INVALID, "okenv_memory_act: " + FRAME_BYTES)
    dev.world_config, dev.memory_config = wc, mc  # (what the binding's own create calls keep for its sizes)
    got, want = memory_act_both(capi, dev, wc, mc, enc, net, ctrl, frames)
    memory_assert_equal(got, want, "the gate opens")
    # a create refused for its config leaves the memory attached, parameterised and acting as before
    refused(dev, h, L.okenv_memory_create(h, None), INVALID, "okenv_memory_create: config is NULL")
    refused(dev, h, L.okenv_memory_create(h, C.byref(capi.memory_config(**dict(memory_mirror.SHAPES["h16"][1], carry=2)))), INVALID,
            "okenv_memory_create: carry must be 0 or 1")
    assert np.abs(got["hidden_state"]).max() > 0 and same(dev.memory_get_hidden(), got["hidden_state"])  # (not zeroed by the refused creates)
    got, want = memory_act_both(capi, dev, wc, mc, enc, net, ctrl, frames)
    memory_assert_equal(got, want, "after the refused creates")
    dev.close()


# ---- 2. growth and reuse of the vectors that are allocated on demand -----------------------------------------------------------------

GROW_N = 17  # two workgroups, one agent in the second


def test_lidar_vector_grows_and_is_reused(gpu):
    """tiny -> a wider 3-point shape (reallocates) -> tiny again (the capacity is kept): after every create the parameters are forgotten,
    and with new ones every slot of the act equals the host entry bit for bit."""
    capi, tiny = gpu.capi, lidar_mirror.SHAPES["tiny"]
    shapes = [tiny, dict(tiny, d_model=32, dim_feedforward=32), tiny]
    dev = population(gpu, GROW_N, 3)
    crashed = dev.get(capi.F_CRASHED)
    rel = np.stack([dev.get(capi.F_REL_X), dev.get(capi.F_REL_Y)], axis=2)
    sizes = []
    for i, shape in enumerate(shapes):
        cfg = capi.lidar_config(**shape)
        params = lidar_mirror.random_params(capi, cfg, np.random.default_rng(20 + i))
        assert dev.lidar_create(cfg) == params.size
        sizes.append(params.size)
        refused(dev, dev._h, dev._L.okenv_lidar_act(dev._h, None), STATE,
                "okenv_lidar_act: call okenv_lidar_set_params first (the policy needs its parameters)")
        dev.lidar_set_params(params)
        rec = {"action": torch.full((GROW_N, 2), -7.0, device="cuda"), "input": torch.full((GROW_N, 3, 2), -7.0, device="cuda"),
               "alive": torch.full((GROW_N,), 9, dtype=torch.uint8, device="cuda")}
        torch.cuda.synchronize()  # the handle has a stream of its own
        dev.lidar_act(rec)
        dev.sync()
        want = capi.lidar_act_host(cfg, params, rel, crashed)
        want["action"] = np.stack([want["throttle"], want["steer"]], axis=1)
        assert same(dev.get(capi.F_THROTTLE), want["throttle"]) and same(dev.get(capi.F_STEER), want["steer"]), i
        for slot, t in rec.items():
            assert same(t.cpu().numpy(), want[slot]), (i, slot)
        assert same(dev.lidar_get_params(), params), i
    assert sizes[1] > sizes[0] == sizes[2]
    dev.close()


def test_flow_vector_grows_and_is_reused(gpu):
    """tiny -> small (reallocates) -> tiny again (the capacity is kept), as for the lidar vector."""
    capi = gpu.capi
    dev = population(gpu, GROW_N, 7)
    crashed = dev.get(capi.F_CRASHED)
    count = dev.step_count
    sizes = []
    for i, name in enumerate(("tiny", "small", "tiny")):
        rng = np.random.default_rng(30 + i)
        cfg = capi.flow_config(seed=13, **flow_mirror.SHAPES[name])
        params = flow_mirror.random_params(capi, cfg, rng)
        cond_host = rng.uniform(-1.0, 1.0, (GROW_N, cfg.cond_dim)).astype(f32)
        cond = torch.from_numpy(cond_host).cuda()
        assert dev.flow_create(cfg) == params.size
        sizes.append(params.size)
        refused(dev, dev._h, dev._L.okenv_flow_act(dev._h, capi.ptr(cond), None), STATE,
                "okenv_flow_act: call okenv_flow_set_params first (the policy needs its parameters)")
        dev.flow_set_params(params)
        rec = {"x0": torch.full((GROW_N, 2), -7.0, device="cuda"), "x": torch.full((GROW_N, 2), -7.0, device="cuda"),
               "action": torch.full((GROW_N, 2), -7.0, device="cuda"), "alive": torch.full((GROW_N,), 9, dtype=torch.uint8, device="cuda")}
        torch.cuda.synchronize()  # the handle has a stream of its own
        dev.flow_act(cond, rec)
        dev.sync()
        want = capi.flow_act_host(cfg, params, cond_host, crashed, draw_index=count)
        want["action"] = np.stack([want["throttle"], want["steer"]], axis=1)
        assert same(dev.get(capi.F_THROTTLE), want["throttle"]) and same(dev.get(capi.F_STEER), want["steer"]), i
        for slot, t in rec.items():
            assert same(t.cpu().numpy(), want[slot]), (i, slot)
        assert same(dev.flow_get_params(), params), i
    assert sizes[1] > sizes[0] == sizes[2]
    dev.close()


# The image families grow more than their vector at create: the conv kernels' pack, the activations that pass through global memory,
# the workspaces.  tiny -> a wider shape of the mirror (everything reallocates) -> tiny again (every capacity is kept, so a capacity or
# a pointer that a shared helper mixed up shows here): after every create the parameters are forgotten, and with new ones the act equals
# the host entry bit for bit in the slots the family's own GPU test compares.

def image_rounds(gpu, names, draw):
    """(handle of GROW_N agents, round, shape name, the round's fresh parameters: draw(name, seed)), the same handle in every round."""
    dev = population(gpu, GROW_N, 3)
    try:
        for i, name in enumerate(names):
            yield dev, i, name, draw(name, 60 + i)
    finally:
        dev.close()


def fields_and_record(dev, capi, rec):
    dev.sync()
    got = {k: t.cpu().numpy() for k, t in rec.items()}
    got.update(throttle=dev.get(capi.F_THROTTLE), steer=dev.get(capi.F_STEER))
    return got


def with_action(want):
    return dict(want, action=np.stack([want["throttle"], want["steer"]], axis=1))


def test_bev_buffers_grow_and_are_reused(gpu):
    capi, sizes = gpu.capi, []
    for dev, i, name, params in image_rounds(gpu, ("tiny", "odd", "tiny"), lambda name, seed: bev_mirror.draw_params(bev_mirror.SHAPES[name], seed)):
        shape = bev_mirror.SHAPES[name]
        cfg, frames = capi.bev_config(**shape), random_frames(GROW_N, shape["image_size"], 60 + i)
        out = torch.full((GROW_N, shape["embed_dim"]), -7.0, device="cuda")
        torch.cuda.synchronize()
        assert dev.bev_create(cfg) == params.size
        sizes.append(params.size)
        refused(dev, dev._h, dev._L.okenv_bev_encode(dev._h, capi.ptr(frames), frames.numel(), capi.ptr(out)), STATE,
                "okenv_bev_encode: call okenv_bev_set_params first (the encoder needs its parameters)")
        dev.bev_set_params(params)
        dev.bev_encode(frames, out)
        dev.sync()
        assert same(out.cpu().numpy(), capi.bev_encode_host(cfg, params, frames.cpu().numpy())), i
        assert same(dev.bev_get_params(), params), i
    assert sizes[1] > sizes[0] == sizes[2]


def test_cnn_buffers_grow_and_are_reused(gpu):
    capi, sizes = gpu.capi, []
    for dev, i, name, params in image_rounds(gpu, ("tiny", "odd", "tiny"), lambda name, seed: cnn_mirror.draw_params(cnn_mirror.SHAPES[name], seed)):
        shape = cnn_mirror.SHAPES[name]
        cfg, frames = capi.cnn_config(throttle=80.0, steer_scale=7.0, **shape), random_frames(GROW_N, shape["image_size"], 60 + i)
        rec = {"out": torch.full((GROW_N,), -7.0, device="cuda"), "action": torch.full((GROW_N, 2), -7.0, device="cuda"),
               "alive": torch.full((GROW_N,), 9, dtype=torch.uint8, device="cuda")}
        torch.cuda.synchronize()
        assert dev.cnn_create(cfg) == params.size
        sizes.append(params.size)
        refused(dev, dev._h, dev._L.okenv_cnn_act(dev._h, capi.ptr(frames), frames.numel(), None), STATE,
                "okenv_cnn_act: call okenv_cnn_set_params first (the policy needs its parameters)")
        dev.cnn_set_params(params)
        dev.cnn_act(frames, rec)
        got = fields_and_record(dev, capi, rec)
        want = with_action(capi.cnn_act_host(cfg, params, frames.cpu().numpy(), dev.get(capi.F_CRASHED)))
        for slot in ("out", "action", "alive", "throttle", "steer"):
            assert same(got[slot], want[slot]), (i, slot)
        assert np.abs(want["out"]).max() > 0
        assert same(dev.cnn_get_params(), params), i
    assert sizes[1] > sizes[0] == sizes[2]


def test_qcnn_buffers_grow_and_are_reused(gpu):
    capi, sizes = gpu.capi, []
    for dev, i, name, params in image_rounds(gpu, ("tiny", "odd", "tiny"), lambda name, seed: qcnn_mirror.draw_params(qcnn_mirror.SHAPES[name], seed)):
        shape = qcnn_mirror.SHAPES[name]
        cfg, frames = qcnn_config(capi, name), random_frames(GROW_N, shape["image_size"], 60 + i)
        rec = {"q": torch.full((GROW_N, shape["num_actions"]), -7.0, device="cuda"), "action": torch.full((GROW_N,), -7, dtype=torch.int64, device="cuda"),
               "value": torch.full((GROW_N,), -7.0, device="cuda"), "alive": torch.full((GROW_N,), 9, dtype=torch.uint8, device="cuda")}
        torch.cuda.synchronize()
        assert dev.qcnn_create(cfg) == params.size
        sizes.append(params.size)
        refused(dev, dev._h, dev._L.okenv_qcnn_act(dev._h, capi.ptr(frames), frames.numel(), None), STATE,
                "okenv_qcnn_act: call okenv_qcnn_set_params first (the network needs its parameters)")
        dev.qcnn_set_params(params)
        dev.qcnn_act(frames, rec)
        got = fields_and_record(dev, capi, rec)
        want = capi.qcnn_act_host(cfg, params, frames.cpu().numpy(), dev.get(capi.F_CRASHED), dev.step_count)
        for slot in ("q", "action", "value", "alive", "throttle", "steer"):
            assert same(got[slot], want[slot]), (i, slot)
        assert np.abs(want["q"]).max() > 0
        assert same(dev.qcnn_get_params(), params), i
    assert sizes[1] > sizes[0] == sizes[2]


def test_world_buffers_grow_and_are_reused(gpu):
    capi, sizes = gpu.capi, []
    for dev, i, name, (enc, ctrl) in image_rounds(gpu, ("tiny", "odd", "tiny"), lambda name, seed: world_mirror.draw_params(world_mirror.SHAPES[name], seed, GROW_N)):
        shape = world_mirror.SHAPES[name]
        cfg, frames = capi.world_config(**shape), random_frames(GROW_N, shape["image_size"], 60 + i)
        rec = world_record(GROW_N, shape["latent"])
        torch.cuda.synchronize()
        assert dev.world_create(cfg) == (enc.size, ctrl.shape[1])
        sizes.append(enc.size)
        unset = "okenv_world_act: call okenv_world_set_params first (the encoder and the controllers need their parameters)"
        refused(dev, dev._h, dev._L.okenv_world_act(dev._h, capi.ptr(frames), frames.numel(), None), STATE, unset)
        dev.world_set_params("controllers", ctrl)
        refused(dev, dev._h, dev._L.okenv_world_act(dev._h, capi.ptr(frames), frames.numel(), None), STATE, unset)  # the encoder is still missing
        dev.world_set_params("encoder", enc)
        dev.world_act(frames, rec)
        got = fields_and_record(dev, capi, rec)
        want = world_host_act(capi, cfg, enc, ctrl, frames, dev)
        for slot in WORLD_RECORD + ("throttle", "steer"):
            assert same(got[slot], want[slot]), (i, slot)
        assert np.abs(want["mu"]).max() > 0.01
        assert same(dev.world_get_params("encoder"), enc) and same(dev.world_get_params("controllers").reshape(ctrl.shape), ctrl), i
    assert sizes[1] > sizes[0] == sizes[2]


def test_memory_buffers_grow_and_are_reused(gpu):
    """h16 on the tiny racers -> h48 on the odd ones -> h16 again: the racers' vector and workspace grow and are reused with the memory's."""
    capi, sizes = gpu.capi, []
    for dev, i, name, (enc, net, ctrl, hidden) in image_rounds(gpu, ("h16", "h48", "h16"), lambda name, seed: memory_drawn(name, seed, GROW_N)):
        wc, mc = memory_configs(capi, name)
        frames = random_frames(GROW_N, wc.image_size, 60 + i)
        dev.world_create(wc)
        dev.world_set_params("encoder", enc)
        assert dev.memory_create(mc) == (net.size, ctrl.shape[1])
        sizes.append(net.size)
        refused(dev, dev._h, dev._L.okenv_memory_act(dev._h, capi.ptr(frames), frames.numel(), None), STATE,
                "okenv_memory_act: call okenv_memory_set_params first (the network and the controllers need their parameters)")
        assert not dev.memory_get_hidden().any()
        dev.memory_set_params("network", net)
        dev.memory_set_params("controllers", ctrl)
        dev.memory_set_hidden(hidden)
        for t in range(2):  # the second act starts from the hidden state the first one left
            got, want = memory_act_both(capi, dev, wc, mc, enc, net, ctrl, frames)
            memory_assert_equal(got, want, "round %d, act %d" % (i, t))
        assert np.abs(got["hidden_state"]).max() > 0.01
        assert same(dev.memory_get_params("network"), net) and same(dev.memory_get_params("controllers").reshape(ctrl.shape), ctrl), i
    assert sizes[1] > sizes[0] == sizes[2]


def test_vit_buffers_grow_and_are_reused(gpu):
    capi, sizes = gpu.capi, []
    configs = {name: capi.vit_config(throttle=80.0, steer_scale=7.0, **vit_mirror.SHAPES[name]) for name in ("tiny", "ten_tokens")}
    draw = lambda name, seed: vit_mirror.random_params(capi, configs[name], np.random.default_rng(seed), scale=2.0)  # noqa: E731
    for dev, i, name, params in image_rounds(gpu, ("tiny", "ten_tokens", "tiny"), draw):
        shape, cfg = vit_mirror.SHAPES[name], configs[name]
        frames = random_frames(GROW_N, shape["image_size"], 60 + i)
        rec = {"action": torch.full((GROW_N, 2), -7.0, device="cuda"), "output": torch.full((GROW_N,), -7.0, device="cuda"),
               "embedding": torch.full((GROW_N, shape["dim"]), -7.0, device="cuda"), "alive": torch.full((GROW_N,), 9, dtype=torch.uint8, device="cuda")}
        torch.cuda.synchronize()
        assert dev.vit_create(cfg) == params.size
        sizes.append(params.size)
        refused(dev, dev._h, dev._L.okenv_vit_act(dev._h, capi.ptr(frames), frames.numel(), None), STATE,
                "okenv_vit_act: call okenv_vit_set_params first (the policy needs its parameters)")
        dev.vit_set_params(params)
        dev.vit_act(frames, rec)
        got = fields_and_record(dev, capi, rec)
        want = with_action(capi.vit_act_host(cfg, params, frames.cpu().numpy(), dev.get(capi.F_CRASHED)))
        for slot in ("action", "output", "embedding", "alive", "throttle", "steer"):
            assert same(got[slot], want[slot]), (i, slot)
        assert np.abs(want["output"]).max() > 0
        assert same(dev.vit_get_params(), params), i
    assert sizes[1] > sizes[0] == sizes[2]


# ---- 3. the families of fixed capacity: what a second create resets ------------------------------------------------------------------

M = 40  # rows of the one update that moves the moments and t before the second create


def rows(rng, R):
    batch = {"state": rng.random((M, R)).astype(f32), "pre": (rng.standard_normal((M, 2)) * 0.7).astype(f32), "logp": (-2.5 - rng.random(M)).astype(f32),
             "ret": rng.standard_normal(M).astype(f32)}
    return {k: torch.from_numpy(v).cuda() for k, v in batch.items()}


def test_second_create_resets_actor(gpu):
    rng = np.random.default_rng(41)
    dev = population(gpu, 3, 5)
    d = rows(rng, 5)
    n_pol, _ = dev.actor_create(8, TABLE)
    dev.actor_set_params((rng.standard_normal(n_pol) * 0.5).astype(f32), None)
    dev.learner_create(lr=0.01)
    dev.reinforce_update({"state": d["state"], "action": torch.from_numpy(rng.integers(0, 3, M).astype(np.int64)).cuda(), "ret": d["ret"]}, M, 64)
    st = dev.learner_state()
    assert st["t"] == 1 and np.abs(st["policy_m"]).max() > 0
    n_pol2, _ = dev.actor_create(12, TABLE)
    assert n_pol2 > n_pol
    refused(dev, dev._h, dev._L.okenv_actor_act(dev._h, None), STATE,
            "okenv_actor_act: call okenv_actor_set_params first (every attached network needs its parameters)")
    t = C.c_int64(-1)
    refused(dev, dev._h, dev._L.okenv_learner_get_state(dev._h, None, None, None, None, C.byref(t)), STATE,
            "okenv_learner_get_state: call okenv_learner_create first")
    policy = (rng.standard_normal(n_pol2) * 0.5).astype(f32)
    dev.actor_set_params(policy, None)
    dev.learner_create(lr=0.01)
    st = dev.learner_state()
    assert st["t"] == 0 and st["policy_m"].size == n_pol2 and not st["policy_m"].any() and not st["policy_v"].any()
    assert same(dev.actor_get_params()[0], policy)
    dev.actor_act()
    dev.sync()
    dev.close()


def test_second_create_resets_ddpg(gpu):
    rng = np.random.default_rng(42)
    N, R = 3, 5
    dev = population(gpu, N, R)
    na, nc = dev.ddpg_create(8, 8)
    dev.ddpg_set_params((rng.standard_normal(na) * 0.3).astype(f32), (rng.standard_normal(nc) * 0.3).astype(f32))
    dev.ddpg_replay_create(16, push_all=True)
    rec = {"state": torch.zeros((N, R), device="cuda"), "action": torch.zeros((N, 2), device="cuda"), "alive": torch.zeros(N, dtype=torch.uint8, device="cuda")}
    torch.cuda.synchronize()
    dev.ddpg_act(rec)
    dev.step(1)
    dev.ddpg_replay_push(rec)
    dev.ddpg_update(4, 1)
    st = dev.ddpg_state()
    assert st["t"] == 1 and np.abs(st["critic_m"]).max() > 0
    na2, nc2 = dev.ddpg_create(12, 10)
    assert na2 > na and nc2 > nc
    refused(dev, dev._h, dev._L.okenv_ddpg_act(dev._h, None), STATE, "okenv_ddpg_act: call okenv_ddpg_set_params first (the actor needs its parameters)")
    actor, critic = (rng.standard_normal(na2) * 0.3).astype(f32), (rng.standard_normal(nc2) * 0.3).astype(f32)
    dev.ddpg_set_params(actor, critic)
    st = dev.ddpg_state()
    assert st["t"] == 0
    for k in ("actor_m", "actor_v", "critic_m", "critic_v"):
        assert st[k].size == (nc2 if "critic" in k else na2) and not st[k].any(), k
    assert same(st["actor"], actor) and same(st["actor_target"], actor) and same(st["critic"], critic) and same(st["critic_target"], critic)
    dev.ddpg_act()
    dev.sync()
    dev.close()


def test_second_create_resets_gauss(gpu):
    rng = np.random.default_rng(43)
    dev = population(gpu, 3, 5)
    d = rows(rng, 5)
    n = dev.gauss_create(8, 8)
    dev.gauss_set_params((rng.standard_normal(n) * 0.3).astype(f32))
    dev.gauss_learner_create(lr=0.01)
    dev.gauss_update({"state": d["state"], "eps": d["pre"], "ret": d["ret"]}, M, 64)
    st = dev.gauss_state()
    assert st["t"] == 1 and np.abs(st["m"]).max() > 0
    n2 = dev.gauss_create(12, 10)
    assert n2 > n
    refused(dev, dev._h, dev._L.okenv_gauss_act(dev._h, None), STATE, "okenv_gauss_act: call okenv_gauss_set_params first (the actor needs its parameters)")
    params = (rng.standard_normal(n2) * 0.3).astype(f32)
    dev.gauss_set_params(params)
    st = dev.gauss_state()
    assert st["t"] == 0 and st["m"].size == n2 and not st["m"].any() and not st["v"].any() and same(st["params"], params)
    dev.gauss_act()
    dev.sync()
    dev.close()


def test_second_create_resets_gcl(gpu):
    rng = np.random.default_rng(44)
    dev = population(gpu, 3, 5)
    d = rows(rng, 5)
    sizes = dev.gcl_create(**GCL_WIDTHS)
    for name, n in sizes.items():
        dev.gcl_set_params(name, (rng.standard_normal(n) * 0.3).astype(f32))
    dev.gcl_learner_create(lr=0.01)
    dev.gcl_policy_update(d, M, 64)
    for name in ("policy", "value"):
        st = dev.gcl_state(name)
        assert st["t"] == 1 and np.abs(st["m"]).max() > 0, name
    sizes2 = dev.gcl_create(hidden1=12, hidden2=10, cost_hidden1=12, cost_hidden2=10)
    refused(dev, dev._h, dev._L.okenv_gcl_act(dev._h, None), STATE, "okenv_gcl_act: call okenv_gcl_set_params first (the policy needs its parameters)")
    for name, n in sizes2.items():
        assert n > sizes[name]
        raw = gpu.capi.OkenvGclState()
        refused(dev, dev._h, dev._L.okenv_gcl_get_state(dev._h, gpu.capi.GCL_NETWORKS[name], C.byref(raw)), STATE,
                "okenv_gcl_get_state: the network needs its parameters first (okenv_gcl_create, okenv_gcl_set_params)")
        params = (rng.standard_normal(n) * 0.3).astype(f32)
        dev.gcl_set_params(name, params)
        st = dev.gcl_state(name)
        assert st["t"] == 0 and st["m"].size == n and not st["m"].any() and not st["v"].any() and same(st["params"], params), name
    dev.gcl_act()
    dev.sync()
    dev.close()


def test_second_create_resets_vit(gpu):
    """okenv_vit_create drops the head's learner: it belonged to the policy that goes."""
    capi = gpu.capi
    dev = population(gpu, 3, 3)
    L, h = dev._L, dev._h
    shape = vit_mirror.SHAPES["tiny"]
    cfg = capi.vit_config(**shape)
    params = vit_mirror.random_params(capi, cfg, np.random.default_rng(46))
    rows = 4
    torch.manual_seed(46)
    embedding, steer = torch.rand((rows, shape["dim"]), device="cuda") - 0.5, torch.rand(rows, device="cuda") - 0.5
    torch.cuda.synchronize()

    def update():
        return L.okenv_vit_head_update(h, capi.ptr(embedding), capi.ptr(steer), rows, rows, 1, None, None)

    dev.vit_create(cfg)
    dev.vit_set_params(params)
    dev.vit_head_learner_create()
    assert update() == OK
    st = dev.vit_head_state()
    assert st["t"] == 1 and np.abs(st["m"]).max() > 0
    dev.vit_create(cfg)
    refused(dev, h, update(), STATE, "okenv_vit_head_update: call okenv_vit_head_learner_create first")
    refused(dev, h, L.okenv_vit_act(h, None, 0, None), STATE, "okenv_vit_act: call okenv_vit_set_params first (the policy needs its parameters)")
    dev.vit_set_params(params)
    refused(dev, h, update(), STATE, "okenv_vit_head_update: call okenv_vit_head_learner_create first")  # parameters do not bring it back
    dev.vit_head_learner_create()
    st = dev.vit_head_state()
    assert st["t"] == 0 and not st["m"].any() and not st["v"].any()
    assert update() == OK
    dev.sync()
    dev.close()


def test_second_create_resets_world(gpu):
    """okenv_world_create detaches the memory, forgets both vectors and zeroes the fitness."""
    capi = gpu.capi
    dev = population(gpu, 3, 3)
    L, h = dev._L, dev._h
    track = gpu.Track("Austin")
    wc, mc = memory_configs(capi, "h16")
    enc, net, ctrl, hidden = memory_drawn("h16", 47, 3)
    racers = world_mirror.draw_params(memory_mirror.shape_of("h16")[0], 47, 3)[1]
    frames = random_frames(3, wc.image_size, 47)
    buf = np.zeros(max(enc.size, racers.size), dtype=f32)
    dev.world_create(wc)
    dev.world_set_params("encoder", enc)
    dev.world_set_params("controllers", racers)
    dev.world_set_lane_widths(track.wl, track.wr)
    dev.world_score_begin()
    dev.world_score()
    assert np.abs(dev.world_fitness()).max() > 0
    dev.memory_create(mc)
    dev.memory_set_params("network", net)
    dev.memory_set_params("controllers", ctrl)
    dev.memory_act(frames)
    dev.world_act(frames)
    dev.sync()
    dev.world_create(wc)
    refused(dev, h, L.okenv_memory_act(h, capi.ptr(frames), frames.numel(), None), STATE, "okenv_memory_act: call okenv_memory_create first")
    refused(dev, h, L.okenv_world_act(h, capi.ptr(frames), frames.numel(), None), STATE,
            "okenv_world_act: call okenv_world_set_params first (the encoder and the controllers need their parameters)")
    for which in (capi.WORLD_ENCODER, capi.WORLD_VECTORS["controllers"]):
        refused(dev, h, L.okenv_world_get_params(h, which, capi.ptr(buf)), STATE,
                "okenv_world_get_params: the vector needs its parameters first (okenv_world_create, okenv_world_set_params)")
    assert not dev.world_fitness().any()
    dev.close()


def test_second_create_resets_memory(gpu):
    """okenv_memory_create forgets both vectors and zeroes the hidden state; the racers keep theirs."""
    capi = gpu.capi
    dev = population(gpu, 3, 3)
    L, h = dev._L, dev._h
    wc, mc = memory_configs(capi, "h16")
    enc, net, ctrl, hidden = memory_drawn("h16", 48, 3)
    frames = random_frames(3, wc.image_size, 48)
    buf = np.zeros(max(net.size, ctrl.size), dtype=f32)
    dev.world_create(wc)
    dev.world_set_params("encoder", enc)
    dev.memory_create(mc)
    dev.memory_set_params("network", net)
    dev.memory_set_params("controllers", ctrl)
    dev.memory_set_hidden(hidden)
    dev.memory_act(frames)
    dev.sync()
    assert dev.memory_get_hidden().any()
    dev.memory_create(mc)
    refused(dev, h, L.okenv_memory_act(h, capi.ptr(frames), frames.numel(), None), STATE,
            "okenv_memory_act: call okenv_memory_set_params first (the network and the controllers need their parameters)")
    for which in (capi.MEMORY_NETWORK, capi.MEMORY_VECTORS["controllers"]):
        refused(dev, h, L.okenv_memory_get_params(h, which, capi.ptr(buf)), STATE,
                "okenv_memory_get_params: the vector needs its parameters first (okenv_memory_create, okenv_memory_set_params)")
    assert not dev.memory_get_hidden().any()
    assert same(dev.world_get_params("encoder"), enc)
    dev.close()


def test_second_create_keeps_or_drops_the_qcnn_ring(gpu):
    """okenv_qcnn_create keeps the frame ring when image_size stays and invalidates it when image_size changes: its planes had the
    earlier network's size."""
    capi = gpu.capi
    dev = population(gpu, 3, 3)
    L, h = dev._L, dev._h
    size, pushed = C.c_int64(-1), C.c_int64(-1)
    refused(dev, h, L.okenv_qcnn_ring_size(h, C.byref(size), C.byref(pushed)), STATE, "okenv_qcnn_ring_size: call okenv_qcnn_ring_create first")
    dev.qcnn_create(qcnn_config(capi, "tiny"))
    dev.qcnn_ring_create(8)
    assert qcnn_mirror.SHAPES["nopad"]["image_size"] == qcnn_mirror.SHAPES["tiny"]["image_size"] != qcnn_mirror.SHAPES["odd"]["image_size"]
    dev.qcnn_create(qcnn_config(capi, "nopad"))
    assert L.okenv_qcnn_ring_size(h, C.byref(size), C.byref(pushed)) == OK and (size.value, pushed.value) == (0, 0)
    dev.qcnn_create(qcnn_config(capi, "odd"))
    refused(dev, h, L.okenv_qcnn_ring_size(h, C.byref(size), C.byref(pushed)), STATE, "okenv_qcnn_ring_size: call okenv_qcnn_ring_create first")
    dev.qcnn_ring_create(8)
    assert L.okenv_qcnn_ring_size(h, C.byref(size), C.byref(pushed)) == OK and (size.value, pushed.value) == (0, 0)
    dev.close()


# ---- 4. host arrays as parameters ----------------------------------------------------------------------------------------------------

def test_host_arrays_as_parameters(gpu):
    """Every family's set_params takes a float64 numpy array, of which the binding makes a float32 temporary that nobody holds once the
    call has returned; the caller's own array is deleted too, and what is read back equals the float32 cast bit for bit.  This pins the
    contract (a host buffer must stay valid until the stream has passed the copy, so the binding waits for the stream when it made the
    buffer).  It is not a reproduction of the lifetime problem, which no test can make deterministic."""
    capi = gpu.capi
    rng = np.random.default_rng(45)
    dev = population(gpu, 3, 3)

    def handed_over(n, give):
        wide = rng.standard_normal(n) * 0.3  # float64
        want = wide.astype(f32)
        give(wide)
        del wide
        return want

    n_pol, n_val = dev.actor_create(8, TABLE, 8)
    policy = handed_over(n_pol, lambda v: dev.actor_set_params(v, None))
    value = handed_over(n_val, lambda v: dev.actor_set_params(None, v))
    got = dev.actor_get_params()
    assert same(got[0], policy) and same(got[1], value)
    na, nc = dev.ddpg_create(8, 8)
    actor = handed_over(na, lambda v: dev.ddpg_set_params(v, None))
    critic = handed_over(nc, lambda v: dev.ddpg_set_params(None, v))
    st = dev.ddpg_state()
    assert same(st["actor"], actor) and same(st["actor_target"], actor) and same(st["critic"], critic) and same(st["critic_target"], critic)
    want = handed_over(dev.gauss_create(8, 8), dev.gauss_set_params)
    assert same(dev.gauss_state()["params"], want)
    for name, n in dev.gcl_create(**GCL_WIDTHS).items():
        want = handed_over(n, lambda v: dev.gcl_set_params(name, v))
        assert same(dev.gcl_state(name)["params"], want), name
    want = handed_over(dev.lidar_create(capi.lidar_config(**lidar_mirror.SHAPES["tiny"])), dev.lidar_set_params)
    assert same(dev.lidar_get_params(), want)
    want = handed_over(dev.flow_create(capi.flow_config(**flow_mirror.SHAPES["tiny"])), dev.flow_set_params)
    assert same(dev.flow_get_params(), want)
    # a strided view is no contiguous array either
    n = dev.gauss_num_params()
    strided = (rng.standard_normal(2 * n) * 0.3).astype(f32)[::2]
    want = strided.copy()
    dev.gauss_set_params(strided)
    del strided
    assert same(dev.gauss_state()["params"], want)
    dev.close()
