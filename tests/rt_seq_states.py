"""Key scripts of the raytracer's Update() (raytracer/Source/skeleton.cpp:192-256) as per-frame
states, shared by test_rt_sequence.py and test_rt_sequence_gpu.py.  Every state is built in
float32, step by step as the keys arrive: the light and the camera move by float32(0.1), the yaw
by float32(0.174533) (so that it returns to exactly 0), the focal length by 10.

This generator is simplified on purpose: its tests compare the GPU with the oracle at whatever
state it makes.  The reference itself steps the yaw in double and narrows to float, so 'm' then 'n'
leaves yaw = -5.372047e-09 there; the states the real program reaches, that one included, are in
tests/golden/ref_sessions.json and rendered by tests/test_ref_sessions_gpu.py."""
import numpy as np

import cgamd
import oracle

F32 = np.float32
LIGHT0 = (0.0, -0.5, -0.7, 1.0)       # skeleton.cpp:86-89
COLOUR0 = (14.0, 14.0, 14.0)
LIGHT_KEYS = {"w": (2, 1), "s": (2, -1), "a": (0, -1), "d": (0, 1), "q": (1, -1), "e": (1, 1)}
CAM_KEYS = {"U": (2, 1), "D": (2, -1), "L": (0, -1), "R": (0, 1)}

# the scripts of the GPU tests: one frame per group of keys (a group may be empty: the start state)
SCRIPT_LIGHT = ["", "dddd", "dddd", "eeeee", "eeeee", "sssss"]      # case 1: the light ends low beside the tall block
SCRIPT_MIXED = list("wUimmaRnnnoqDe")                               # case 3


def pitch(a):
    """A rotation about x (as tests/test_routes.py: pitch): R turns y, so the frame goes per pixel."""
    c, s = float(np.cos(F32(a), dtype=F32)), float(np.sin(F32(a), dtype=F32))
    m = [1.0 if k % 5 == 0 else 0.0 for k in range(16)]
    m[5], m[6], m[9], m[10] = c, s, -s, c
    return (cgamd.C.c_float * 16)(*m)


class State:
    def __init__(self, cam, focal, yaw, light, keys):
        self.cam, self.focal, self.yaw, self.light, self.keys = cam, focal, yaw, light, keys

    def R(self):
        """None for the identity (yaw exactly 0: Update() never touched R, or cos = 1, sin = 0)."""
        return cgamd.yaw_matrix(float(self.yaw)) if float(self.yaw) != 0.0 else None

    def lights(self, colour=COLOUR0):
        return [(self.light, colour)]


def key_states(groups, focal, cam=(0.0, 0.0, -3.0, 1.0), light=LIGHT0):
    cam = [F32(x) for x in cam]
    light = [F32(x) for x in light]
    yaw, focal = F32(0.0), F32(focal)
    out = []
    for g in groups:
        for k in g:
            if k in LIGHT_KEYS:
                ax, sg = LIGHT_KEYS[k]
                light[ax] = F32(light[ax] + F32(sg) * F32(0.1))
            elif k in CAM_KEYS:
                ax, sg = CAM_KEYS[k]
                cam[ax] = F32(cam[ax] + F32(sg) * F32(0.1))
            elif k in "nm":
                yaw = F32(yaw + (F32(-0.174533) if k == "n" else F32(0.174533)))
            elif k in "io":
                focal = F32(focal + (F32(10) if k == "i" else F32(-10)))
            else:
                raise ValueError(k)
        out.append(State(tuple(float(x) for x in cam), float(focal), yaw, tuple(float(x) for x in light), g))
    return out


def cross_states(n=35):
    """Case 2: light and cameraPos change every frame (small steps, so 35 frames stay in the room)."""
    out = []
    for f in range(n):
        cam = (float(F32(0.01) * F32(f - n // 2)), 0.0, float(F32(-3.0) + F32(0.01) * F32(f)), 1.0)
        light = (float(F32(-0.4) + F32(0.025) * F32(f)), -0.5, float(F32(-0.7) + F32(0.01) * F32(f)), 1.0)
        out.append(State(cam, 45.0, F32(0.0), light, "*"))
    return out


def camera(st, W, H):
    return cgamd.rt_camera(W, H, st.focal, st.cam, st.R())


def light_array(lights):
    arr = (cgamd.Light * len(lights))()
    for i, (p, c) in enumerate(lights):
        arr[i].position = cgamd.Vec4(*p)
        arr[i].colour = cgamd.Vec3(*c)
    return arr


def oracle_frame(st, W, H, lights=None, scene=None, threads=8):
    R = st.R()
    p = oracle.rt_params(W, H, st.focal, st.cam, list(R) if R is not None else None,
                         lights=lights if lights is not None else st.lights())
    return oracle.rt_draw(p, threads=threads, scene=scene)
