"""The robot-side wire format of the reference's `use_lcm` path (controllers/basic_controller.py:52-61,79-87,289-314):
`robot_state_control_lcmt` messages (lcm_types/robot_state_control_lcmt.lcm: float q[19], v[18], tau[12]; 204 bytes).

  decode_robot_state / encode_robot_state     one message on the host (the C codec of libwbc_hip.so, no `lcm` needed)
  unpack_states(messages)                     N "robot_current_state" messages -> q[19, N], v[18, N] on the device
  pack_controls(tau, q_perm, act_perm)        tau[12, N] (actuator order, as wbc_step writes it) -> N
                                              "robot_control_input" messages: tau = (S'u)[-12:] in the plant's joint
                                              order, q and v zero -- what basic_controller.py:308-314 publishes

Transport (LCM sockets, channels) is out of scope; these are the bytes either side of the tick, batched.
Bit-exact against the reference's own generated codec (tests/golden/make_robot_state_golden.py)."""
import ctypes as C

import numpy as np

from . import _lib

MESSAGE_BYTES = 204


def decode_robot_state(buf):
    """bytes -> dict(q [19], v [18], tau [12]) of float32 values; ValueError("Decode error") on a foreign fingerprint."""
    s = _lib.WbcRobotState()
    rc = _lib.lib().wbc_robot_state_decode(bytes(buf), len(buf), C.byref(s))
    if rc != 0:
        raise ValueError("Decode error" if rc == -3 else "short robot_state_control_lcmt buffer")
    return dict(q=np.array(s.q[:], dtype=np.float32), v=np.array(s.v[:], dtype=np.float32), tau=np.array(s.tau[:], dtype=np.float32))


def encode_robot_state(q=None, v=None, tau=None):
    """-> 204 bytes; values are rounded to float32 (round to nearest even, like the reference's struct.pack('>f'))."""
    s = _lib.WbcRobotState()
    for name, n, val in (("q", 19, q), ("v", 18, v), ("tau", 12, tau)):
        a = np.zeros(n, dtype=np.float32) if val is None else np.asarray(val, dtype=np.float64).reshape(n).astype(np.float32)
        getattr(s, name)[:] = a.tolist()
    out = C.create_string_buffer(MESSAGE_BYTES)
    if _lib.lib().wbc_robot_state_encode(C.byref(s), out, MESSAGE_BYTES) != MESSAGE_BYTES:
        raise ValueError("encode failed")
    return out.raw


_OWNER = "the codec"


def unpack_states(messages, device=0, out=None):
    """messages: bytes / list of bytes / uint8 CUDA tensor [N * 204] -> (q [19, N], v [18, N], ok [N] uint8) on the device,
    asynchronously on torch's current stream.  ok[i] = 0: foreign fingerprint, that robot's columns are left as they were."""
    import torch
    if not isinstance(messages, torch.Tensor):
        raw = messages if isinstance(messages, (bytes, bytearray)) else b"".join(messages)
        messages = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to("cuda:%d" % device)
    n, rest = divmod(messages.numel(), MESSAGE_BYTES)
    if rest:
        raise ValueError("messages: a contiguous uint8 CUDA tensor (or bytes) holding whole 204-byte messages")
    pm = _lib.dev_ptr(messages, 0, n * MESSAGE_BYTES, "uint8", "messages", device, _OWNER)
    (q, v), (pq, pv) = _lib.outputs(out, ((19, "float64", "q"), (18, "float64", "v")), n, device, _OWNER, zero=True)
    (ok,), (pok,) = _lib.outputs(None, ((0, "uint8", "ok"),), n, device, _OWNER)
    _lib.check(_lib.lib().wbc_robot_states_unpack(device, C.c_void_p(_lib.stream_of(device)), n, n, pm, pq, pv, pok))
    return q, v, ok


def pack_controls(tau, q_perm=None, act_perm=None):
    """tau: float64 CUDA tensor [12, N] in actuator order -> uint8 CUDA tensor [N * 204] of "robot_control_input" messages."""
    import torch
    if not (isinstance(tau, torch.Tensor) and tau.is_cuda and tau.dim() == 2):
        raise ValueError("tau: a contiguous float64 CUDA tensor [12, N]")
    n, device = int(tau.shape[1]), tau.device.index
    pt = _lib.dev_ptr(tau, 12, n, "float64", "tau", device, _OWNER)
    (msgs,), (pm,) = _lib.outputs(None, ((0, "uint8", "messages"),), n * MESSAGE_BYTES, device, _OWNER)
    arr = lambda p: None if p is None else (C.c_int * 12)(*[int(x) for x in p])
    _lib.check(_lib.lib().wbc_robot_controls_pack(device, C.c_void_p(_lib.stream_of(device)), n, n, pt, arr(q_perm), arr(act_perm), pm))
    return msgs
