"""The drivers' life cycle on the host ("The drivers' life cycle on the host"): create, num_params, set_params, get_params /
get_state, set_draw_offset, set_greedy and act of the six families that attach a network to the handle (actor, DDPG, Gaussian actor,
guided cost learning, lidar transformer, flow matching).  What okenv_last_error says is public API: every refusal's return code and
exact text, per entry and in the entry's own order of checks; the growth and reuse of the two vectors that are allocated on demand;
what a second create resets; host arrays as parameters."""
import ctypes as C

import numpy as np
import pytest
import torch

import _flow_numpy as flow_mirror
import _lidar_numpy as lidar_mirror
from test_gpu_lidar import same  # the predicate of test_gpu_lidar.py and test_gpu_flow.py: same shape, same bytes

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
    """One handle of 3 agents and 3 rays for the refusals of all six families: each test touches its own family only."""
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
