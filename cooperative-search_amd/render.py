"""Episode frames: the state (and map) rows of recorded episodes as RGB pictures (include/coopsearch.h: cs_render_episodes).

`render_episodes_torch` is the DEFINITION of a frame, in stock torch ops (it runs on the CPU); the kernel (csrc/render.h)
reproduces it byte for byte, and `render_episodes` sends device tensors to the kernel and host tensors to the definition.
DESIGN.md section 15 has the text of the definition; in short, with W = spec.size and U = 16 W sub-units across the map:

  quantisation  qx = rint((xn + 1) * 8W), qy = U - rint((yn + 1) * 8W)  (image row 0 is the top of the map), ci = rint(cos * 1024),
                si = rint(sin * 1024) -- float32, one add or one multiply then round-half-even; everything after is integer.
                A target is found when its flag is > 0.5.  Pixel (row r, column c) has its centre at X = 16c + 8, Y = 16r + 8.
  layers        background (white, or the heat colour of the map cell under the pixel) -> sensor discs (blended) -> trails ->
                sensor rings -> targets (unfound, then found) -> agents (triangles along the heading) -> progress bar; a later
                layer overwrites an earlier one.
  frames        frame t of episode e is drawn from row min(t, clamp(counts[e], 1, R) - 1): padded steps repeat the last real
                frame and rows past the count are never read.

Rows that no env emits are made harmless rather than undefined: a quantised position is clamped to +-2^20 sub-units and a
heading component to +-1024 (NaN goes to the lower bound), and a triangle only covers pixels within max(L, L//2 + 6L//10)
sub-units of its agent per axis -- no vertex is further -- so a row with cos = sin = 0 paints that box, not the image.  None of
the three changes a frame of rows that get_state() produces.
"""
import dataclasses
import os

import numpy as np
import torch

from . import _lib

HEAT, SENSOR, TRAIL, TARGETS, AGENTS, BAR = 1, 2, 4, 8, 16, 32   # CS_RENDER_* of include/coopsearch.h
POS_LIM = float(1 << 20)
PALETTE = ((214, 39, 40), (31, 119, 180), (44, 160, 44), (148, 103, 189), (140, 86, 75), (227, 119, 194), (23, 190, 207),
           (188, 189, 34))


def _default_lut():
    """256 x 3: white at 0 through yellow and red to a dark red at 1, integer arithmetic only."""
    stops = ((0, (255, 255, 255)), (85, (255, 237, 160)), (170, (240, 59, 32)), (255, (103, 0, 13)))
    out = bytearray()
    for v in range(256):
        for (v0, c0), (v1, c1) in zip(stops, stops[1:]):
            if v0 <= v <= v1:
                out += bytes((c0[ch] * (v1 - v) + c1[ch] * (v - v0) + (v1 - v0) // 2) // (v1 - v0) for ch in range(3))
                break
    return bytes(out)


DEFAULT_LUT = _default_lut()


@dataclasses.dataclass(frozen=True)
class RenderSpec:
    """What a frame looks like.  size: W, a multiple of 4 in 16..1024; view_range / map_size: the sensor radius as a fraction of
    the map; n_agents: how many (xn, yn, cos, sin) groups lead a state row (the rest are targets); the six layer switches;
    colours as (r, g, b); palette: 8 colours, agent i's trail and triangle; lut: 768 bytes, the heat colour of
    rint(clamp(p, 0, 1) * 255)."""
    size: int = 256
    view_range: float = 7
    map_size: float = 50
    n_agents: int = 3
    heat: bool = True
    sensor: bool = True
    trail: bool = True
    targets: bool = True
    agents: bool = True
    bar: bool = True
    background: tuple = (255, 255, 255)
    sensor_tint: tuple = (100, 149, 237)
    sensor_ring: tuple = (65, 105, 225)
    target: tuple = (0, 0, 0)
    target_found: tuple = (255, 165, 0)
    bar_on: tuple = (46, 160, 67)
    bar_off: tuple = (211, 211, 211)
    palette: tuple = PALETTE
    lut: bytes = DEFAULT_LUT

    def __post_init__(self):
        if int(self.size) != self.size or self.size % 4 or not 16 <= self.size <= 1024:
            raise ValueError(f"RenderSpec: size must be a multiple of 4 in 16..1024, got {self.size!r}")
        if not 1 <= int(self.n_agents) <= _lib.MAX_AGENTS:
            raise ValueError(f"RenderSpec: n_agents must be 1..{_lib.MAX_AGENTS}, got {self.n_agents!r}")
        if len(self.palette) != 8 or len(bytes(self.lut)) != 768:
            raise ValueError("RenderSpec: palette must hold 8 colours and lut 256 x 3 bytes")
        for c in self.colours() + [ch for p in self.palette for ch in p]:
            if not 0 <= int(c) <= 255:
                raise ValueError("RenderSpec: a colour channel is outside 0..255")
        if not self.map_size > 0 or not 0 <= self.radii()[0] <= 32767:
            raise ValueError("RenderSpec: view_range / map_size must give a sensor radius of 0..32767 sub-units")

    @classmethod
    def for_env(cls, env, size=256, **kw):
        """The spec of an env's (or an args namespace's) team and sensor."""
        return cls(size=int(size), view_range=env.view_range, map_size=env.map_size, n_agents=int(env.n_agents), **kw)

    @property
    def U(self):
        return 16 * int(self.size)

    def radii(self):
        """(rv, rt, rtr, L) in sub-units, Python ints: sensor, target disc, trail, triangle length."""
        U = self.U
        return (int(round(self.view_range / self.map_size * U)), max(16, int(round(0.012 * U))), max(8, int(round(0.006 * U))),
                int(round(0.03 * U)))

    def layers(self):
        return sum(bit for bit, on in ((HEAT, self.heat), (SENSOR, self.sensor), (TRAIL, self.trail), (TARGETS, self.targets),
                                       (AGENTS, self.agents), (BAR, self.bar)) if on)

    def colours(self):
        """7 x (r, g, b), flat, in the op's order."""
        return [int(ch) for c in (self.background, self.sensor_tint, self.sensor_ring, self.target, self.target_found, self.bar_on,
                                  self.bar_off) for ch in c]

    def n_targets(self, state_width):
        n = int(self.n_agents)
        m, rest = divmod(int(state_width) - 4 * n, 3)
        if rest or not 1 <= m <= _lib.MAX_TARGETS:
            raise ValueError(f"a state row of {state_width} floats is not 4 x {n} agents + 3 x (1..{_lib.MAX_TARGETS}) targets")
        return m


def _pack(rgb):
    return int(rgb[0]) | (int(rgb[1]) << 8) | (int(rgb[2]) << 16)


def _quant(v, lim):
    """rint(v) as int64 in [-lim, lim]; NaN gives -lim."""
    r = torch.round(v)
    hi, lo = torch.full_like(r, lim), torch.full_like(r, -lim)
    return torch.where(r >= -lim, torch.where(r <= lim, r, hi), lo).to(torch.int64)


def _check_tables(states, maps, counts, spec):
    if states.dim() != 3 or states.dtype != torch.float32:
        raise ValueError("states must be float32 [E, R, 4n + 3m]")
    E, R, S = (int(v) for v in states.shape)
    m = spec.n_targets(S)
    if E < 1 or R < 1:
        raise ValueError("states must hold at least one episode of at least one row")
    side = 0
    if maps is not None:
        side = int(round(float(maps.shape[-1]) ** 0.5)) if maps.dim() == 3 else 0
        if maps.dtype != torch.float32 or maps.dim() != 3 or tuple(maps.shape[:2]) != (E, R) or side * side != int(maps.shape[2]) \
                or not 1 <= side <= 64:
            raise ValueError("maps must be float32 [E, R, side * side] with side 1..64")
    if counts.dim() != 1 or int(counts.shape[0]) != E or counts.dtype not in (torch.int32, torch.int64):
        raise ValueError("counts must be int32 / int64 [E]")
    return E, R, S, m, side


def _render_episode(st, mp, spec, m, side):
    """One episode whose rows are already the frames' rows: st float32 [R, S], mp float32 [R, side^2] or None -> uint8
    [R, W, W, 3]."""
    i64 = torch.int64
    dev = st.device
    R, n, W, U = int(st.shape[0]), int(spec.n_agents), int(spec.size), spec.U
    rv, rt, rtr, L = spec.radii()
    h, w = L // 2, (L * 6) // 10
    tb = max(L, h + w)
    s8w = float(8 * W)
    ag = st[:, :4 * n].reshape(R, n, 4)
    tg = st[:, 4 * n:].reshape(R, m, 3)
    ax, ay = _quant((ag[..., 0] + 1.0) * s8w, POS_LIM), U - _quant((ag[..., 1] + 1.0) * s8w, POS_LIM)
    ci, si = _quant(ag[..., 2] * 1024.0, 1024.0), _quant(ag[..., 3] * 1024.0, 1024.0)
    tx, ty = _quant((tg[..., 0] + 1.0) * s8w, POS_LIM), U - _quant((tg[..., 1] + 1.0) * s8w, POS_LIM)
    found = tg[..., 2] > 0.5                                   # [R, m]
    k = found.sum(1).to(i64)                                   # [R]
    P = 16 * torch.arange(W, dtype=i64, device=dev) + 8        # pixel centres along either axis
    X, Y = P.view(1, 1, W), P.view(1, W, 1)

    def const(rgb):
        return torch.tensor(_pack(rgb), dtype=i64, device=dev)

    pal = [const(c) for c in spec.palette]
    # (a) background
    if spec.heat and mp is not None:
        ix = torch.clamp(torch.div(P * side, U, rounding_mode="floor"), 0, side - 1)
        iy = torch.clamp(torch.div((U - P) * side, U, rounding_mode="floor"), 0, side - 1)
        cell = (ix.view(1, W) * side + iy.view(W, 1)).reshape(-1)          # [row, column] -> ix * side + iy
        p = mp.index_select(1, cell)
        pc = torch.where(p > 0.0, torch.where(p < 1.0, p, torch.ones_like(p)), torch.zeros_like(p))
        lut = torch.frombuffer(bytearray(bytes(spec.lut)), dtype=torch.uint8).view(256, 3).to(dev).to(i64)
        lut = lut[:, 0] | (lut[:, 1] << 8) | (lut[:, 2] << 16)
        col = lut[torch.round(pc * 255.0).to(i64)].view(R, W, W)
    else:
        col = const(spec.background).expand(R, W, W).clone()
    dxa = [X - ax[:, i].view(R, 1, 1) for i in range(n)]
    dya = [Y - ay[:, i].view(R, 1, 1) for i in range(n)]
    d2a = [dxa[i] * dxa[i] + dya[i] * dya[i] for i in range(n)]            # [R, W, W] int64
    # (b) sensor fill
    if spec.sensor:
        fill = d2a[0] <= rv * rv
        for i in range(1, n):
            fill = fill | (d2a[i] <= rv * rv)
        blend = torch.zeros_like(col)
        tint = _pack(spec.sensor_tint)
        for ch in range(3):
            blend = blend | (torch.div(96 * ((tint >> (8 * ch)) & 255) + 159 * ((col >> (8 * ch)) & 255) + 127, 255,
                                       rounding_mode="floor") << (8 * ch))
        col = torch.where(fill, blend, col)
    # (c) trails: everywhere agent i has been up to this frame
    if spec.trail:
        for i in range(n):
            seen = torch.cummax((d2a[i] <= rtr * rtr).to(torch.uint8), 0).values.to(torch.bool)
            col = torch.where(seen, pal[i], col)
    # (d) sensor ring
    if spec.sensor:
        ring = torch.zeros_like(fill)
        for i in range(n):
            ring = ring | ((d2a[i] > (rv - 16) * (rv - 16)) & (d2a[i] <= rv * rv))
        col = torch.where(ring, const(spec.sensor_ring), col)
    # (e) targets: the unfound ones, then the found ones
    if spec.targets:
        unf = torch.zeros(R, W, W, dtype=torch.bool, device=dev)
        fnd = torch.zeros(R, W, W, dtype=torch.bool, device=dev)
        for j in range(m):
            dx, dy = X - tx[:, j].view(R, 1, 1), Y - ty[:, j].view(R, 1, 1)
            disc = dx * dx + dy * dy <= rt * rt
            f = found[:, j].view(R, 1, 1)
            unf, fnd = unf | (disc & ~f), fnd | (disc & f)
        col = torch.where(unf, const(spec.target), col)
        col = torch.where(fnd, const(spec.target_found), col)
    # (f) agents: triangles in sub-units x 1024
    if spec.agents:
        PX, PY = 1024 * X, 1024 * Y
        for i in range(n):
            bx, by = (1024 * ax[:, i]).view(R, 1, 1), (1024 * ay[:, i]).view(R, 1, 1)
            c, s = ci[:, i].view(R, 1, 1), si[:, i].view(R, 1, 1)
            v0x, v0y = bx + L * c, by - L * s
            v1x, v1y = bx - h * c + w * s, by + h * s + w * c
            v2x, v2y = bx - h * c - w * s, by + h * s - w * c
            e0 = (v1x - v0x) * (PY - v0y) - (v1y - v0y) * (PX - v0x)
            e1 = (v2x - v1x) * (PY - v1y) - (v2y - v1y) * (PX - v1x)
            e2 = (v0x - v2x) * (PY - v2y) - (v0y - v2y) * (PX - v2x)
            inside = ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))
            inside = inside & (dxa[i].abs() <= tb) & (dya[i].abs() <= tb)
            col = torch.where(inside, pal[i], col)
    # (g) progress bar
    if spec.bar:
        on = torch.arange(W, dtype=i64, device=dev).view(1, W) * m < k.view(R, 1) * W
        col[:, :4, :] = torch.where(on, const(spec.bar_on), const(spec.bar_off)).view(R, 1, W)
    return torch.stack([((col >> (8 * ch)) & 255).to(torch.uint8) for ch in range(3)], -1)


def frame_rows(counts, R):
    """int64 [E, R]: the row frame t of episode e is drawn from, min(t, clamp(counts[e], 1, R) - 1)."""
    last = counts.to(torch.int64).clamp(1, R) - 1
    return torch.minimum(torch.arange(R, dtype=torch.int64, device=counts.device).view(1, R), last.view(-1, 1))


def render_episodes_torch(states, maps, counts, spec):
    """The definition of a frame (module docstring): states float32 [E, R, 4n + 3m], maps float32 [E, R, side^2] or None,
    counts int32 / int64 [E] -> uint8 [E, R, W, W, 3] on the tensors' device.  Rows past an episode's count are not read."""
    E, R, S, m, side = _check_tables(states, maps, counts, spec)
    rows = frame_rows(counts, R)
    W = int(spec.size)
    out = torch.empty(E, R, W, W, 3, dtype=torch.uint8, device=states.device)
    for e in range(E):
        mp = None if maps is None else maps[e].index_select(0, rows[e])
        out[e] = _render_episode(states[e].index_select(0, rows[e]), mp, spec, m, side)
    return out


_device_tables = {}


def _palette_lut(spec, device):
    """uint8 [8, 3] and [256, 3] of a spec on a device, made once."""
    key = (spec.palette, bytes(spec.lut), str(device))
    if key not in _device_tables:
        pal = torch.tensor([[int(ch) for ch in c] for c in spec.palette], dtype=torch.uint8)
        lut = torch.frombuffer(bytearray(bytes(spec.lut)), dtype=torch.uint8).view(256, 3)
        _device_tables[key] = (pal.to(device), lut.to(device))
    return _device_tables[key]


def render_episodes(states, maps, counts, spec, out=None):
    """Frames of E episodes, uint8 [E, R, W, W, 3] (written into `out` when given).  Device tensors go to the kernel
    (torch.ops.coopsearch.render_episodes on the current stream; nothing synchronises once a spec's palette and lookup table
    are on the device), host tensors to `render_episodes_torch`."""
    if not states.is_cuda:
        frames = render_episodes_torch(states, maps, counts, spec)
        if out is None:
            return frames
        out.copy_(frames)
        return out
    E, R, S, m, side = _check_tables(states, maps, counts, spec)
    W = int(spec.size)
    if out is None:
        out = torch.empty(E, R, W, W, 3, dtype=torch.uint8, device=states.device)
    pal, lut = _palette_lut(spec, states.device)
    if counts.dtype != torch.int32:
        counts = counts.to(torch.int32)
    ops = _lib.torch_ops_for("episode frames need")
    ops.render_episodes(states, maps, counts, int(spec.n_agents), m, side, W, list(spec.radii()), spec.layers(), spec.colours(), pal, lut, out)
    return out


def episode_tables(batch, args=None, with_maps=True):
    """(states [E, T+1, S], maps [E, T+1, cells] or None, counts int32 [E]) of an episode batch, float32.  A dense batch (the
    reference's 11 keys): row 0 is s[:, 0] and row t + 1 is s_next[:, t]; the map (observations wider than 4 floats) is agent
    0's part of o / o_next.  A map-once batch (replay.COMPACT_KEYS): s_full and map as they are.  counts = real steps + 1,
    computed where the batch lives (no host read).  with_maps=False: maps is None and no map is copied (sweep.sweep_batch)."""
    f32 = torch.float32
    if "s_full" in batch:
        states, maps = batch["s_full"].to(f32), batch["map"].to(f32) if with_maps else None
    else:
        states = torch.cat([batch["s"][:, :1], batch["s_next"]], 1).to(f32)
        cells = int(batch["o"].shape[-1]) - 4
        if args is not None and bool(getattr(args, "conv", cells > 0)) != (cells > 0):
            raise ValueError(f"episode_tables: observations of {cells + 4} floats do not fit args.conv = {args.conv!r}")
        maps = torch.cat([batch["o"][:, :1, 0, :cells], batch["o_next"][:, :, 0, :cells]], 1).to(f32) if cells > 0 and with_maps else None
    counts = ((1 - batch["padded"].to(f32)).sum(1).reshape(-1) + 1).to(torch.int32)
    return states.contiguous(), None if maps is None else maps.contiguous(), counts


def _tile(frames):
    """[K, H, W, 3] -> one [rows * H, cols * W, 3] sheet, cols = ceil(sqrt(K)), white where no picture is."""
    K, H, W = frames.shape[:3]
    cols = int(np.ceil(np.sqrt(K)))
    rows = (K + cols - 1) // cols
    sheet = np.full((rows * H, cols * W, 3), 255, dtype=np.uint8)
    for i in range(K):
        r, c = divmod(i, cols)
        sheet[r * H:(r + 1) * H, c * W:(c + 1) * W] = frames[i]
    return sheet


def write_frames(frames, path, duration=80):
    """Frames to a file; returns the path written.  uint8 [E, R, W, W, 3] (or [R, W, W, 3] with a path ending in .gif): an
    animated GIF of R pictures, the E episodes side by side; uint8 [K, W, W, 3]: one PNG contact sheet.  Without PIL: the array
    itself as `path + ".npy"`.  duration: milliseconds per GIF picture."""
    arr = frames.detach().cpu().numpy() if torch.is_tensor(frames) else np.asarray(frames)
    if arr.dtype != np.uint8 or arr.ndim not in (4, 5) or arr.shape[-1] != 3:
        raise ValueError("write_frames: frames must be uint8 [E, R, W, W, 3] or [K, W, W, 3]")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    try:
        from PIL import Image
    except ImportError:
        np.save(path + ".npy", arr)
        return path + ".npy"
    if arr.ndim == 4 and not path.lower().endswith(".gif"):
        path = path if path.lower().endswith(".png") else path + ".png"
        Image.fromarray(_tile(arr)).save(path, format="PNG")
        return path
    if arr.ndim == 4:
        arr = arr[None]
    path = path if path.lower().endswith(".gif") else path + ".gif"
    pics = [Image.fromarray(_tile(arr[:, t])) for t in range(arr.shape[1])]
    pics[0].save(path, format="GIF", save_all=True, append_images=pics[1:], duration=int(duration), loop=0)
    return path
