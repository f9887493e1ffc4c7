"""The protocol of tests/test_scripted_play_gpu.py, stated once: scripted agents that play all seven games — bossfight, chaser,
climber, caveflyer, coinrun, jumper and maze — to win on the CPU oracle.  The GPU half feeds their actions to the HIP engine
beside the oracle; tests/test_scripted_play.py runs the protocol on the oracle alone and asserts that it reaches the ground
random play never does (the boss's six phases and its death, cleared boards, levels with every coin collected, caveflyer's
destroyed targets, its full bullet ring and more sprites than a wavefront has lanes, the second half of coinrun's levels with
its lava, crates dropped through and levels deep in an env's chain, jumper's memory world far from the start), so the GPU
tests are known not to be vacuous before a GPU is touched.

A policy is a pure function of (the oracle's state dump, the oracle's tile dump, step, env, a seeded numpy Generator) that
returns an action.  It reads the ORACLE's dumps, never the engine's: the test stays valid if the engine's state rows are wrong,
and a divergence shows as a byte mismatch at the step where it happens.  Columns are named through the layout the project
states (pgv_state_layout_of / pgv_state_names: host-only), never by bare index.

Lock-step protocol: N = 65 envs (one wavefront and one lane: the second wavefront is all but empty), seed_base 17, the
engine's own auto-reset, no masked resets, STEPS[(game, mode)] steps.  Events are counted from the oracle's dumps and outputs
(Counter), and assert_covers holds the floors.
"""
import ctypes
import functools
import math

import numpy as np

from test_modes import EASY, EXTREME, HARD, MEMORY, TABLE  # noqa: F401

GAMES = ("bossfight", "chaser", "climber", "caveflyer", "coinrun", "jumper", "maze")
PAIRS = [(g, m) for g in GAMES for m in sorted(TABLE[g][1])]  # 18
N, SEED_BASE, POLICY_SEED = 65, 17, 9
# The fewest steps (rounded up to the next 50) after which the oracle's run holds every floor of assert_covers; the step at
# which the last floor is reached: bossfight 684 / 732, chaser 1023 / 954 / 1429, climber 140 / 152, caveflyer 251 (the
# turning turret's full turn) / 284 (the fifth step with a target's 3.0) / 212 (a full turn), coinrun 250 / 250 (an env's
# eighth ended episode), jumper 227 / 214 / 203 (5 000 env-steps with no jump left), maze 53 / 77 / 105 (the twentieth first
# step of a sixth or later level), steps counted from 0.
STEPS = {("bossfight", EASY): 700, ("bossfight", HARD): 750, ("chaser", EASY): 1050, ("chaser", HARD): 1000,
         ("chaser", EXTREME): 1450, ("climber", EASY): 200, ("climber", HARD): 200,
         ("caveflyer", EASY): 300, ("caveflyer", HARD): 300, ("caveflyer", MEMORY): 250,
         ("coinrun", EASY): 300, ("coinrun", HARD): 300, ("jumper", EASY): 250, ("jumper", HARD): 250, ("jumper", MEMORY): 250,
         ("maze", EASY): 100, ("maze", HARD): 100, ("maze", MEMORY): 150}
# chaser's modes that fall back from a cleared board to an episode that ate at least 85 % of its points and orbs
ATE_85_INSTEAD = {("chaser", EXTREME)}
RARE_ENVS = 8  # state and tile rows are compared in at most this many envs a step

LEFT, NOOP, RIGHT, UP, DOWN, JUMP_LEFT, JUMP_RIGHT, FIRE = 1, 4, 7, 3, 5, 2, 8, 9  # (up and down: chaser's; world y grows with 3)
ORB, POINT, EGG = 0, 1, 2   # chaser's record kinds (oracle/pgo_chaser.cpp)
HATCH_TIME = 50.0
WALL = 1                    # chaser's wall tile; climber's walls are every non-zero tile


class Columns:
    """A game's state row by name: f[name] a fixed column, r[name] the offset inside a record."""

    def __init__(self, lay, unlisted=()):
        self.f = {name: i for i, name in enumerate(lay.fixed_names)}
        self.r = {name: i for i, name in enumerate(lay.record_names)}
        self.fixed, self.record, self.width = lay.fixed, lay.record, lay.width
        self.cells, self.tile_w, self.tile_h = lay.cells, lay.tile_w, lay.tile_h
        self.unlisted = tuple(unlisted)  # the things the row has no record of: their scalars describe them
        assert len(self.f) == lay.fixed and len(self.r) == lay.record

    def count(self, st):
        """The records of a row: one a thing, but for the unlisted ones among the row's n_things."""
        n = int(st[self.f["n_things" if "n_things" in self.f else "n_spikes"]])  # (jumper's records are its spikes)
        return n - sum(1 for thing in self.unlisted if thing < n)

    def records(self, st):
        k = self.count(st)
        return st[self.fixed:self.fixed + k * self.record].reshape(k, self.record)

    def slots(self, prefix, field):
        """The fixed columns prefix0_field, prefix1_field, … of a row's slot table, in slot order."""
        out = []
        while "%s%d_%s" % (prefix, len(out), field) in self.f:
            out.append(self.f["%s%d_%s" % (prefix, len(out), field)])
        return out


UNLISTED = {"caveflyer": (1,)}  # the ship is entity 1 and has no record (oracle/pgo_caveflyer.cpp dump_state)


@functools.lru_cache(maxsize=None)
def columns(game, mode):
    from engine_util import pglib
    return Columns(pglib.state_layout(pglib.load(), game, mode), UNLISTED.get(game, ()))


class Dumps:
    """Every env's oracle dumps at one point: states float32 [n, width] (+0.0 behind a dump), tiles uint8 [n, cells]."""

    def __init__(self, ora, c):
        n = ora.n
        self.states = np.zeros((n, c.width), np.float32)
        self.lengths = np.zeros(n, np.int32)
        self.tiles = np.zeros((n, max(1, c.cells)), np.uint8)
        fp, bp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint8)
        s0, t0, dump_state, dump_tiles, h = self.states.ctypes.data, self.tiles.ctypes.data, ora.L.pgo_vec_dump_state, ora.L.pgo_vec_dump_tiles, ora.h
        for e in range(n):
            self.lengths[e] = got = dump_state(h, e, ctypes.cast(s0 + e * c.width * 4, fp), c.width)
            assert 0 < got <= c.width, (e, got)
            assert "n_things" not in c.f or got == c.fixed + c.record * c.count(self.states[e]), (e, got)
            if c.cells:
                assert dump_tiles(h, e, ctypes.cast(t0 + e * c.cells, bp), c.cells) == c.cells

    def state(self, e):
        return self.states[e, :self.lengths[e]]


# ---------------------------------------------------------------------------------------------------------- the policies

def bossfight_policy(c, st, tiles, step, env, rng):
    """Steps aside from live boss bullets close to the ship, follows the boss's x and fires while the shield is down,
    otherwise fires 30 % of the time.  Every fourth env does not dodge: the run keeps its deaths."""
    f = c.f
    u = rng.random()
    ax, ay, bx = float(st[f["agent_x"]]), float(st[f["agent_y"]]), float(st[f["boss_x"]])
    first = f["b_shot0_x"]
    shots = st[first:first + 64 * 3].reshape(64, 3)
    dx, dy = shots[:, 0] - ax, ay - shots[:, 1]
    near = (shots[:, 2] == 0) & (np.abs(dx) < 0.45) & (dy > -0.2) & (dy < 0.6)
    if env % 4 != 3 and near.any():
        k = int(np.argmin(np.where(near, np.abs(dx) + np.abs(dy), np.inf)))
        go = LEFT if dx[k] >= 0 else RIGHT
        if ax < -1.6:
            go = RIGHT
        elif ax > 1.6:
            go = LEFT
        return go
    if int(st[f["phase_index"]]) % 2 == 1:
        if abs(bx - ax) < 0.35:
            return FIRE
        return RIGHT if bx > ax else LEFT
    return FIRE if u < 0.3 else NOOP


@functools.lru_cache(maxsize=None)
def _neighbours(W, H):
    """cell → ((cell beside it, its action), …), a cell being y + x * H.  Tile row y - 1 is world y + 1: action 3."""
    out = []
    for x in range(W):
        for y in range(H):
            out.append(tuple((c, a) for ok, c, a in ((x > 0, y + (x - 1) * H, LEFT), (x < W - 1, y + (x + 1) * H, RIGHT),
                                                     (y > 0, y - 1 + x * H, UP), (y < H - 1, y + 1 + x * H, DOWN)) if ok))
    return tuple(out)


FAR = 10 ** 6
ORB_WHEN = 3
BOLD_EVERY, BOLD_FOR = 50, 12
HORIZON = 5  # chaser looks out for enemies this many steps ahead; they turn at random half the time


def _field(nb, wall, sources):
    """Steps from the nearest of `sources` to every cell, through cells that are no wall; FAR where there is no way."""
    dist = [FAR] * len(nb)
    frontier = list(sources)
    for c in frontier:
        dist[c] = 0
    d = 0
    while frontier:
        d += 1
        nxt = []
        for c in frontier:
            for p, _ in nb[c]:
                if dist[p] == FAR and not wall[p]:
                    dist[p] = d
                    nxt.append(p)
        frontier = nxt
    return dist


def _walk(nb, wall, start, targets, enemy, limit=FAR, horizon=HORIZON):
    """Breadth-first from `start` through cells the agent reaches well before an enemy can (an enemy is a quarter faster):
    (the action of the first step towards the nearest cell of `targets`, or None; the action towards the reached cell that
    is safest when it is reached, or None)."""
    seen = {start}
    frontier = [(start, None)]
    d, best, flee = 0, enemy[start] if enemy[start] < FAR else FAR, None
    while frontier and d < limit:
        d += 1
        nxt = []
        for c, first in frontier:
            for p, a in nb[c]:
                if p in seen or wall[p] or (d <= horizon and enemy[p] <= 1.25 * d + 1.5):
                    continue
                seen.add(p)
                if p in targets:
                    return first or a, flee
                slack = enemy[p] - 1.25 * d
                if slack > best:
                    best, flee = slack, first or a
                nxt.append((p, first or a))
        frontier = nxt
    return None, flee


def _cell(x, y, H):
    return (H - 1 - int(math.floor(y))) + int(math.floor(x)) * H


def chaser_policy(c, st, tiles, step, env, rng):
    """Between two cells, with no enemy within 4, it keeps going.  Otherwise it walks to the nearest point by breadth-first
    search through the cells it reaches well before a hatched (or nearly hatched) enemy can; an orb counts as a point when an
    enemy is within 3 steps or no point is left; with an orb's timer running it hunts the hatched enemies within 10 steps
    first; with nowhere safe to go it makes for the cell it reaches with the most to spare, then away from the enemies, then
    on regardless."""
    f, r = c.f, c.r
    W, H = c.tile_w, c.tile_h
    rng.random()
    ax, ay = float(st[f["agent_x"]]), float(st[f["agent_y"]])
    vx, vy = float(st[f["agent_vel_x"]]), float(st[f["agent_vel_y"]])
    rec = c.records(st)
    powered = float(st[f["eat_timer"]]) > 10.0
    kind = rec[:, r["kind"]]
    eggs = rec[(kind == EGG) & (rec[:, r["alive"]] != 0)]
    threat = eggs[eggs[:, r["hatch_timer"]] >= HATCH_TIME - 12]
    if (vx != 0 or vy != 0) and max(abs(ax - math.floor(ax) - 0.5), abs(ay - math.floor(ay) - 0.5)) > 0.11:
        if powered or not len(threat) or (np.abs(threat[:, r["x"]] - ax) + np.abs(threat[:, r["y"]] - ay)).min() > 4.5:
            return RIGHT if vx > 0 else LEFT if vx < 0 else UP if vy > 0 else DOWN
    nb = _neighbours(W, H)
    wall = (tiles == WALL).tolist()
    start = _cell(ax, ay, H)

    def cells_of(rows):
        at = (H - 1 - np.floor(rows[:, r["y"]]).astype(int)) + np.floor(rows[:, r["x"]]).astype(int) * H
        return set(at[(at >= 0) & (at < W * H)].tolist())
    food = rec[(kind != EGG) & (rec[:, r["alive"]] != 0)]
    points, orbs = cells_of(food[food[:, r["kind"]] == POINT]), cells_of(food[food[:, r["kind"]] == ORB])
    if powered:
        enemy = [FAR] * (W * H)
        hatched = cells_of(eggs[eggs[:, r["hatch_timer"]] >= HATCH_TIME])
        if hatched:
            go, _ = _walk(nb, wall, start, hatched, enemy, limit=min(10, int(float(st[f["eat_timer"]]) * 0.08)))
            if go is not None:
                return go
    else:
        enemy = _field(nb, wall, cells_of(threat))
    targets = points | orbs if not points or enemy[start] <= ORB_WHEN else points
    bold = (step + 7 * env) % BOLD_EVERY < BOLD_FOR  # (a stand-off with enemies that hover at the mouth of a dead end is broken in time)
    go, flee = _walk(nb, wall, start, targets, enemy, horizon=1 if bold else HORIZON)
    if go is None and orbs and not powered:
        go, flee = _walk(nb, wall, start, orbs, enemy)
    if go is None:
        go = flee
    if go is None:  # nothing is safe: the neighbour farther from the enemies, or on regardless
        best = enemy[start]
        for p, a in nb[start]:
            if not wall[p] and enemy[p] > best:
                best, go = enemy[p], a
    if go is None:
        go, _ = _walk(nb, wall, start, points | orbs, [FAR] * (W * H))
    return NOOP if go is None else go


def climber_policy(c, st, tiles, step, env, rng):
    """Goes for the lowest coin.  On its level it walks to it; below a coin it walks to the column beside the end of the next
    platform up (the lowest row of wall above the one it stands on), waits while a mob is near the way up, and jumps towards
    the platform; in the air it steers onto the platform."""
    f, r = c.f, c.r
    W, H = c.tile_w, c.tile_h
    rng.random()
    ax, ay, vx = float(st[f["agent_x"]]), float(st[f["agent_y"]]), float(st[f["agent_vel_x"]])
    ground = st[f["agent_ground"]] != 0
    rec = c.records(st)
    alive = rec[:, r["alive"]] != 0
    is_mob = alive & (rec[:, r["vel_x"]] != 0)
    is_coin = alive & (rec[:, r["vel_x"]] == 0)
    if not is_coin.any():
        return NOOP
    grid = tiles.reshape(W, H) != 0  # grid[x, row], row 0 the floor; world y = H - 1 - row at a tile's top
    feet = min(H - 1, max(0, H - 1 - int(math.floor(ay))))
    stand = 0
    for col in {int(math.floor(ax - 0.49)), int(math.floor(ax + 0.49))}:
        col = min(W - 1, max(0, col))
        below = np.nonzero(grid[col, :feet + 1])[0]
        stand = max(stand, int(below[-1]) if below.size else 0)
    body = stand + 1
    coins = rec[is_coin]
    coin_rows = H - 1 - np.floor(coins[:, r["y"]]).astype(int)
    lowest = coin_rows.min()
    pick = coins[coin_rows == lowest]
    coin_x = float(pick[np.argmin(np.abs(pick[:, r["x"]] - ax)), r["x"]])
    above = np.nonzero(grid[1:W - 1, stand + 1:].any(axis=0))[0]
    if lowest <= body or above.size == 0 or stand + 1 + int(above[0]) >= H - 1:
        return RIGHT if coin_x > ax else LEFT
    row = stand + 1 + int(above[0])
    span = np.nonzero(grid[1:W - 1, row])[0] + 1
    lo, hi = int(span[0]), int(span[-1])
    best = None
    for col, way in ((lo - 1, 1), (hi + 1, -1)):
        if not 1 <= col <= W - 2:
            continue
        ok = bool(grid[col, stand]) and not grid[col, stand + 1:row + 2].any()
        cost = abs(col + 0.5 - ax) + (0 if ok else 100)
        if best is None or cost < best[0]:
            best = (cost, col, way)
    _, col, way = best
    tx = col + 0.5
    if not ground:
        if ay < H - 1 - stand - 0.05:  # off the ground: onto the platform
            return RIGHT if way > 0 else LEFT
        return RIGHT if tx > ax else LEFT
    if abs(ax - tx) <= 0.3:
        mobs = rec[is_mob]
        mob_rows = H - 1 - np.floor(mobs[:, r["y"]]).astype(int)
        if ((mob_rows >= body) & (mob_rows <= row + 2) & (np.abs(mobs[:, r["x"]] - (tx + 0.6 * way)) < 2.2)).any():
            return NOOP
        if vx * way >= -0.01:
            return JUMP_RIGHT if way > 0 else JUMP_LEFT
        return RIGHT if way > 0 else LEFT
    return RIGHT if tx > ax else LEFT


# caveflyer (oracle/pgo_caveflyer.cpp agent_update): actions 0-2 turn the ship clockwise and 6-8 counter-clockwise by 0.05 a
# step, 2 / 5 / 8 thrust along the nose, 0 / 3 / 6 thrust backwards at half strength, 9 fires (and does nothing else)
SPIN_CW, SPIN_CCW, SPIN_CW_THRUST, THRUST, SPIN_CCW_THRUST, SPIN_CW_BACK, BACK, SPIN_CCW_BACK = 1, 7, 2, 5, 8, 0, 3, 6
METEOR, TARGET, ENEMY, GOAL = 0, 1, 2, 3  # caveflyer's record kinds
CRUISE = 0.3          # the speed the navigator asks for: the ship's own limit under thrust is 0.5 cells a step
SIGHT = 12.0          # a target this far along the nose, in cells, is shot at
HUNT_WITHIN = 6.0     # the hunter turns onto targets this near, in cells
HUNT_EVERY, HUNT_FOR = 120, 80  # … for this many steps of every so many: a target behind a meteor is given up in time
NAVIGATOR, HUNTER, GUNNER, TURRET = 0, 1, 2, 3  # caveflyer's roles, by env % 4


@functools.lru_cache(maxsize=256)
def _cave_fields(tiles, W, H, goal, hazards):
    """Steps to `goal` from every cell of a caveflyer level (`tiles`: the tile dump's bytes), three times: through cells
    that are neither a hazard's nor beside one, through cells that are no hazard's, through every cell that is no wall.  A
    level's fields change only when a target is destroyed, so they are kept by what they were made from."""
    nb = _neighbours(W, H)
    wall = [t == WALL for t in tiles]
    wide = list(wall)
    narrow = list(wall)
    for cell in hazards:
        narrow[cell] = wide[cell] = True
        for p, _ in nb[cell]:
            wide[p] = True
    narrow[goal] = wide[goal] = False
    return _field(nb, wide, (goal,)), _field(nb, narrow, (goal,)), _field(nb, wall, (goal,))


def _turn(angle):
    """`angle` brought into [-pi, pi)."""
    return (angle + math.pi) % (2.0 * math.pi) - math.pi


def _clear_line(tiles, H, W, ax, ay, bx, by):
    """No wall on the straight line between two points, looked at every quarter of a cell."""
    n = max(1, int(4.0 * math.hypot(bx - ax, by - ay)))
    for k in range(1, n + 1):
        x, y = ax + (bx - ax) * k / n, ay + (by - ay) * k / n
        if not (0 <= x < W and 0 <= y < H) or tiles[_cell(x, y, H)] == WALL:
            return False
    return True


@functools.lru_cache(maxsize=256)
def _longest_line(tiles, W, H, ax, ay):
    """The heading, of 64, along which a bullet from (ax, ay) flies farthest before it meets a wall (`tiles`: the dump's bytes)."""
    best = (-1, 0.0)
    for k in range(64):
        heading = k * math.pi / 32.0
        ux, uy = 0.25 * math.cos(heading), 0.25 * math.sin(heading)
        n, x, y = 0, ax, ay
        while 0 <= x < W and 0 <= y < H and tiles[_cell(x, y, H)] != WALL:
            n, x, y = n + 1, x + ux, y + uy
        best = max(best, (n, heading))
    return best[1]


def caveflyer_policy(c, st, tiles, step, env, rng):
    """Four roles by env % 4.  The navigator flies down a breadth-first field from the goal's cell — through cells that are
    not beside a meteor or a target while such a way exists — at CRUISE cells a step, pushed aside by whatever hazard comes
    near: it turns the nose (or the tail) onto the change of velocity it wants and thrusts when that is within reach, and
    fires when a target lies on the line of fire.  The hunter is the navigator, but turns onto a target in sight within
    HUNT_WITHIN cells first, braking as it turns.  The gunner is the navigator firing every other step.  The turret never
    thrusts, and comes in three kinds by (env // 4) % 3: one fires and turns one way, step about (the ring fills while
    agent_rot passes a full turn); one only fires; one turns onto the nearest target in sight, then onto the longest free
    line there is from where it stands, and fires along it (what fills the ring of 32)."""
    f, r = c.f, c.r
    W, H = c.tile_w, c.tile_h
    rng.random()
    role, turret = env % 4, (env // 4) % 3
    if role == TURRET and turret == 0:
        return SPIN_CCW if step % 2 == 1 else FIRE
    if role == TURRET and turret == 1:
        return FIRE
    ax, ay, rot = float(st[f["agent_x"]]), float(st[f["agent_y"]]), float(st[f["agent_rot"]])
    vx, vy = float(st[f["agent_vel_x"]]), float(st[f["agent_vel_y"]])
    nose_x, nose_y = math.cos(rot), math.sin(rot)
    rec = c.records(st)
    live = rec[rec[:, r["alive"]] != 0]
    kind = live[:, r["kind"]]
    goal, hazards = live[kind == GOAL], live[kind != GOAL]
    fixed = hazards[hazards[:, r["kind"]] != ENEMY]
    if not len(goal):
        return NOOP

    # a target on the line of fire: shoot it
    targets = hazards[hazards[:, r["kind"]] == TARGET]
    dx, dy = targets[:, r["x"]] - ax, targets[:, r["y"]] - ay
    along, off = dx * nose_x + dy * nose_y, dx * nose_y - dy * nose_x
    for k in np.nonzero((along > 0.5) & (along < SIGHT) & (np.abs(off) < 0.2))[0]:
        if _clear_line(tiles, H, W, ax, ay, ax + float(dx[k]), ay + float(dy[k])):
            return FIRE
    if role == GUNNER and step % 2 == 1:
        return FIRE
    if role == TURRET or (role == HUNTER and (step + 13 * env) % HUNT_EVERY < HUNT_FOR):
        near = np.hypot(dx, dy)
        for k in np.argsort(near):
            if near[k] > (SIGHT if role == TURRET else HUNT_WITHIN):
                break
            if _clear_line(tiles, H, W, ax, ay, ax + float(dx[k]), ay + float(dy[k])):
                to = _turn(math.atan2(float(dy[k]), float(dx[k])) - rot)
                slide = vx * nose_x + vy * nose_y  # the hunter brakes what it can while it turns
                if role == HUNTER and abs(slide) > 0.02:
                    return (SPIN_CCW_BACK if to > 0 else SPIN_CW_BACK) if slide > 0 else (SPIN_CCW_THRUST if to > 0 else SPIN_CW_THRUST)
                return SPIN_CCW if to > 0 else SPIN_CW
    if role == TURRET:
        to = _turn(_longest_line(tiles.tobytes(), W, H, ax, ay) - rot)
        return FIRE if abs(to) < 0.03 else SPIN_CCW if to > 0 else SPIN_CW

    # the velocity it wants: down the field, and away from what is near
    def cells_of(rows):
        return (H - 1 - np.floor(rows[:, r["y"]]).astype(int)) + np.floor(rows[:, r["x"]]).astype(int) * H
    start = _cell(ax, ay, H)
    fields = _cave_fields(tiles.tobytes(), W, H, int(cells_of(goal)[0]), tuple(sorted(set(cells_of(fixed).tolist()))))
    field = next((d for d in fields if d[start] < FAR), None)
    want_x = want_y = 0.0
    if field is not None and field[start] > 0:
        nb = _neighbours(W, H)
        at = start
        for _ in range(2):
            at = min((p for p, _ in nb[at]), key=lambda p: field[p]) if field[at] > 0 else at
        to_x, to_y = at // H + 0.5 - ax, H - 1 - at % H + 0.5 - ay
        far = math.hypot(to_x, to_y)
        want_x, want_y = CRUISE * to_x / max(far, 1e-6), CRUISE * to_y / max(far, 1e-6)
    elif field is not None:
        want_x, want_y = float(goal[0, r["x"]]) - ax, float(goal[0, r["y"]]) - ay
    hx, hy = ax - hazards[:, r["x"]], ay - hazards[:, r["y"]]
    reach = np.where(hazards[:, r["kind"]] == ENEMY, 2.5, 1.4)
    dist = np.hypot(hx, hy)
    push = np.where(dist < reach, (reach - dist) / reach, 0.0) / np.maximum(dist, 1e-6)
    want_x += 0.6 * float((push * hx).sum())
    want_y += 0.6 * float((push * hy).sum())

    # the change of velocity, and the nose or the tail onto it
    need_x, need_y = want_x - vx, want_y - vy
    if math.hypot(need_x, need_y) < 0.03:
        return NOOP
    to = _turn(math.atan2(need_y, need_x) - rot)
    if abs(to) <= 0.5 * math.pi:
        if abs(to) < 0.03:
            return THRUST
        if abs(to) < 0.9:
            return SPIN_CCW_THRUST if to > 0 else SPIN_CW_THRUST
        return SPIN_CCW if to > 0 else SPIN_CW
    to = _turn(to - math.pi)
    if abs(to) < 0.03:
        return BACK
    if abs(to) < 0.9:
        return SPIN_CCW_BACK if to > 0 else SPIN_CW_BACK
    return SPIN_CCW if to > 0 else SPIN_CW


# coinrun (oracle/pgo_coinrun.cpp tick_agent): 6-8 move right and 0-2 left, 2 / 5 / 8 jump when grounded, 0 / 3 / 6 ("down") let
# the agent through the crate it stands on.  World y grows downward; agent_y is the feet, the body the cell above them.
CR_WALLS, CR_LAVA, CR_CRATE, CR_STANDS = (1, 2), (3, 4), 5, (1, 2, 5)
CR_DOWN, CR_JUMP = 3, 5
RUNNER, RUNNER_TOO, CRATE_WALKER, HOPPER = 0, 1, 2, 3  # coinrun's roles, by env % 4
CR_JUMP_SPEED, CR_GRAVITY, CR_SPEED, CR_AIR_MIX = 1.55, 0.2, 0.5, 0.2 * 0.15
CRATE_REACH = 8       # the crate walker looks this many columns ahead for a pile to land on
CRATE_RISE = 5.0      # … whose top is at most this far above its feet (a jump rises 6 cells)
LAND_WITHIN = 0.3     # … and jumps when it can come down this near the pile's middle


def _cr_tile(tiles, W, H, x, row):
    """Tile (x, row), row counted downward as the world's y is; a wall outside the map."""
    if x < 0 or row < 0 or x >= W or row >= H:
        return 2
    return int(tiles[(H - 1 - row) + x * H])


def _cr_lands(vx, vy, move, rise):
    """How far along x a coinrun agent in the air comes down onto a surface `rise` cells above its feet (below them when
    negative) while it holds `move` (-1, 0, 1); None when it never gets that high.  The tick's own arithmetic, in doubles,
    nothing in the way."""
    x = y = 0.0
    above = rise < 0
    for _ in range(4 * 48):
        vx += CR_AIR_MIX * (CR_SPEED * move - vx) * 0.25
        vy = min(vy + CR_GRAVITY * 0.25, CR_JUMP_SPEED)
        x += vx * 0.25
        y += vy * 0.25
        if y < -rise:
            above = True
        elif vy > 0:
            return x if above else None
    return None


def _cr_runner_jumps(c, st, tiles, ax, ay):
    """The runner's rule: a wall in the body's row within two columns, no floor under the next column, lava in the feet's row
    or the one below within two columns, or a hazard (every record but the last, the coin) 0 to 3 cells ahead and within 2
    cells of the body's height."""
    W, H, r = c.tile_w, c.tile_h, c.r
    x, feet = int(math.floor(ax)), int(round(ay))
    body = feet - 1
    if any(_cr_tile(tiles, W, H, x + k, body) in CR_WALLS for k in (1, 2)):
        return True
    if _cr_tile(tiles, W, H, x + 1, feet) not in CR_STANDS:
        return True
    if any(_cr_tile(tiles, W, H, x + k, row) in CR_LAVA for k in (1, 2) for row in (feet, feet + 1)):
        return True
    rec = c.records(st)[:-1]
    dx, dy = rec[:, r["x"]] - ax, rec[:, r["y"]] - (ay - 0.5)
    return bool(((dx >= 0) & (dx <= 3) & (np.abs(dy) <= 2)).any())


def on_crate(c, st, tiles):
    """A coinrun row whose agent is grounded with a crate under its feet."""
    f = c.f
    if st[f["agent_ground"]] == 0:
        return False
    ax, feet = float(st[f["agent_x"]]), int(round(float(st[f["agent_y"]])))
    return any(_cr_tile(tiles, c.tile_w, c.tile_h, col, feet) == CR_CRATE for col in {int(math.floor(ax - 0.49)), int(math.floor(ax + 0.49))})


def coinrun_policy(c, st, tiles, step, env, rng):
    """Four roles by env % 4.  Two runners hold RIGHT and jump, when grounded, by the rule of _cr_runner_jumps.  The crate
    walker is a runner that presses down for the step when it stands on a crate (the one-way fall-through), and seeks the
    crates: with a pile within CRATE_REACH columns ahead whose top it can reach, it speeds up or brakes until a jump from
    where it stands comes down on the pile, jumps, and steers onto it in the air (the flight is worked out from the tick's
    own numbers); the runner's rule comes first.  The hopper plays JUMP_RIGHT and nothing else: it is the one that dies."""
    f = c.f
    W, H = c.tile_w, c.tile_h
    rng.random()
    role = env % 4
    if role == HOPPER:
        return JUMP_RIGHT
    ax, ay = float(st[f["agent_x"]]), float(st[f["agent_y"]])
    ground = st[f["agent_ground"]] != 0
    if role != CRATE_WALKER:
        return JUMP_RIGHT if ground and _cr_runner_jumps(c, st, tiles, ax, ay) else RIGHT
    if on_crate(c, st, tiles):
        return CR_DOWN
    vx, vy = float(st[f["agent_vel_x"]]), float(st[f["agent_vel_y"]])
    if ground and _cr_runner_jumps(c, st, tiles, ax, ay):
        return JUMP_RIGHT
    # the nearest pile ahead: its column's topmost crate with nothing on it, its top within reach above the feet
    x0 = int(math.floor(ax))
    for col in range(x0 + 1, min(W - 1, x0 + CRATE_REACH) + 1):
        rows = np.nonzero(tiles[col * H:(col + 1) * H] == CR_CRATE)[0]
        if not rows.size:
            continue
        top = H - 1 - int(rows[-1])  # the row of the topmost crate: its upper edge is world y = top
        rise, to = ay - top, col + 0.5 - ax
        if rise > CRATE_RISE or to < 0.3 or (ground and rise < 0.5):
            continue
        if ground:
            near, far = (_cr_lands(vx, -CR_JUMP_SPEED, move, rise) for move in (-1, 1))
            if to > far + LAND_WITHIN:
                return RIGHT
            if to < near - LAND_WITHIN:
                return LEFT if vx > 0.02 else NOOP
            return JUMP_RIGHT if to > 0.5 * (near + far) else CR_JUMP
        lands = [(abs(x - to), a) for x, a in ((_cr_lands(vx, vy, move, rise), a) for move, a in ((1, RIGHT), (0, NOOP), (-1, LEFT))) if x is not None]
        if lands:
            return min(lands)[1]
        break
    return RIGHT


@functools.lru_cache(maxsize=512)
def _goal_field(tiles, W, H, goal, walls):
    """Steps to the cell `goal` from every cell of a level (`tiles`: the tile dump's bytes) through cells whose tile is not
    among `walls`; kept by what it was made from, so once a level."""
    return _field(_neighbours(W, H), [t in walls for t in tiles], (goal,))


# jumper (oracle/pgo_jumper.cpp agent_update): 6-8 right, 0-2 left, 2 / 5 / 8 jump — twice off the ground, the second when
# agent_jump_timer (3 steps) has run out.  agent_y is the feet; the body is 0.5 wide and 0.8 high.
JP_WALLS = (1, 2)
JP_CENTRED = 0.15      # a vertical move is made from this near the column's middle
JP_SPIKE_AHEAD = 1.6   # a spike this near ahead at body height is jumped over
JP_WANDER_EVERY, JP_WANDER_FOR = 48, 10  # an env that has to go up walks sideways, jumping, for so many steps of every so many


def jumper_policy(c, st, tiles, step, env, rng):
    """Down a breadth-first field from the goal's cell over the cells that are no wall (kept per level), gravity left out:
    to the neighbour that is nearer, sideways before down before up.  For a vertical move it centres on the column to within
    JP_CENTRED, and for one upward it jumps whenever a jump is to be had.  Every env but the fourth of four jumps over a
    spike within JP_SPIKE_AHEAD cells ahead at body height; the fourth keeps the spike deaths.  The way out for an env that
    stands under a ledge it cannot jump onto: while the move is upward, JP_WANDER_FOR steps of every JP_WANDER_EVERY (shifted
    by env) go sideways, jumping, one way or the other by turns."""
    f = c.f
    W, H = c.tile_w, c.tile_h
    rng.random()
    ax, ay = float(st[f["agent_x"]]), float(st[f["agent_y"]])
    can_jump = st[f["agent_jumps"]] > 0 and st[f["agent_jump_timer"]] == 0
    field = _goal_field(tiles.tobytes(), W, H, _cell(float(st[f["goal_x"]]), float(st[f["goal_y"]]), H), JP_WALLS)
    x, y = min(W - 1, max(0, int(math.floor(ax)))), min(H - 1, max(0, H - 1 - int(math.floor(ay - 0.4))))
    here = field[y + x * H]
    # (tile row y + 1 is the cell above: the world's y grows downward, the tile rows count upward)
    ways = [(field[y + (x + dx) * H], 0, dx, 0) for dx in (1, -1) if 0 <= x + dx < W]
    ways += [(field[y + dy + x * H], 1 if dy < 0 else 2, 0, dy) for dy in (-1, 1) if 0 <= y + dy < H]
    best = min(ways)
    if best[0] >= here:  # nowhere nearer (a cell the field does not reach): towards the goal as the crow flies
        best = (0, 0, 1 if st[f["goal_x"]] > ax else -1, 0)
    _, _, dx, dy = best
    off = x + 0.5 - ax
    if dy:
        if dy > 0 and (step + 11 * env) % JP_WANDER_EVERY < JP_WANDER_FOR:
            return (JUMP_RIGHT if can_jump else RIGHT) if ((step + 11 * env) // JP_WANDER_EVERY + env) % 2 else (JUMP_LEFT if can_jump else LEFT)
        if abs(off) > JP_CENTRED:
            return RIGHT if off > 0 else LEFT
        return CR_JUMP if dy > 0 and can_jump else NOOP
    if env % 4 != 3 and can_jump:
        spikes = c.records(st)
        ahead, high = (spikes[:, 0] - ax) * dx, spikes[:, 1] - (ay - 0.4)
        if ((ahead > 0) & (ahead <= JP_SPIKE_AHEAD) & (np.abs(high) < 0.8)).any():
            return JUMP_RIGHT if dx > 0 else JUMP_LEFT
    return RIGHT if dx > 0 else LEFT


MZ_WALLS = (1,)


def maze_policy(c, st, tiles, step, env, rng):
    """Down the breadth-first field from the goal's cell (kept per level).  Every fourth env plays the field's move two steps
    in three and a move into a wall otherwise (the refused move); where no wall is beside it, the field's move."""
    f = c.f
    W, H = c.tile_w, c.tile_h
    rng.random()
    field = _goal_field(tiles.tobytes(), W, H, _cell(float(st[f["goal_x"]]), float(st[f["goal_y"]]), H), MZ_WALLS)
    here = _cell(float(st[f["agent_x"]]), float(st[f["agent_y"]]), H)
    nb = _neighbours(W, H)[here]
    if env % 4 == 3 and step % 3 == 2:
        taken = {a for p, a in nb if tiles[p] not in MZ_WALLS}
        for a in (LEFT, UP, RIGHT, DOWN):
            if a not in taken:
                return a
    near, go = min((field[p], a) for p, a in nb)
    return go if near < field[here] else NOOP


POLICIES = {"bossfight": bossfight_policy, "chaser": chaser_policy, "climber": climber_policy, "caveflyer": caveflyer_policy,
            "coinrun": coinrun_policy, "jumper": jumper_policy, "maze": maze_policy}


def choose_actions(game, mode, dumps, step, rng):
    """The scripted action of every env, in env order, from the oracle's dumps before the step."""
    c, policy = columns(game, mode), POLICIES[game]
    return np.array([policy(c, dumps.states[e], dumps.tiles[e], step, e, rng) for e in range(dumps.states.shape[0])], np.int32)


# ---------------------------------------------------------------------------------------------------- events and floors

LANES = 64                 # of a wavefront: caveflyer's render wave draws one thing a lane while everything fits
FULL_TURN = 2.0 * math.pi  # caveflyer: the ship's rotation is never wrapped


def cave_draws(c, sprites, shots):
    """What a caveflyer frame draws behind its tiles, from the row's own numbers: every puff slot, the live sprites, the
    bullets of the ring that count, the ship."""
    return len(c.slots("puff", "life")) + sprites + shots + 1


class Counter:
    """Events of a run, counted from the oracle's dumps before and after every step and from its reward and done rows.  The
    engine's own auto-reset is the next step's: an env that ended keeps its terminal state in the dump after that step, and
    its next step (whatever the action) installs the next level and counts for nothing here."""

    def __init__(self, game, mode, n):
        self.game, self.mode, self.c = game, mode, columns(game, mode)
        self.counts = dict(wins=0, deaths=0, ends=0)
        self.rare, self.after = [], None  # the envs in a rare state after the last step counted, and that step's dumps
        self.first = True
        self.resetting = np.zeros(n, bool)  # the envs whose next step is their reset step
        if game == "bossfight":
            self.counts.update(phases=set(), damaged=0, win_and_death_steps=0)
        if game == "climber":
            self.counts.update(coins=0, wins_with_3_coins=0, rewards_11=0, most_coins_in_a_win=0)
            self.level_coins = np.zeros(n, int)
            self.lost_coin = np.zeros(n, bool)
        if game == "chaser":
            self.counts.update(eaten_enemies=0, wins_or_85=0, best_share=0.0)
            self.board = np.zeros(n, int)
            self.ate_85 = np.zeros(n, bool)
        if game == "caveflyer":
            self.counts.update(target_steps=0, targets_destroyed=0, double_target_steps=0, goal_with_target_steps=0, most_shots=0, steps_over_8=0,
                               steps_over_16=0, steps_over_24=0, ring_full_steps=0, overflow_steps=0, most_turn=0.0)
            self.hit_target = np.zeros(n, bool)
        self.turns = 0
        if game in ("coinrun", "jumper", "maze"):
            self.counts.update(most_ends=0, deep_starts=0)
            self.env_ends = np.zeros(n, int)  # the episodes every env has ended: its level is number env_ends + 1
        if game == "coinrun":
            self.counts.update(lava_deaths=0, saw_deaths=0, mob_deaths=0, other_deaths=0, env_steps=0, past_half=0, past_09=0, crate_steps=0, drop_steps=0,
                               envs_with_3_ends=0)
            self.dropped = np.zeros(n, bool)
        if game == "jumper":
            self.counts.update(no_jump_steps=0, no_jump_timer_steps=0, envs_with_no_end=n)
            if mode == MEMORY:
                self.counts.update(farthest=0.0, octants=set(), most_octants_in_an_env=0)
                self.env_octants = np.zeros((n, 8), bool)
            self.began_at = np.zeros((n, 2))
        if game == "maze":
            self.counts.update(median_ends=0, longest_episode=0)
            self.length = np.zeros(n, int)

    def coinrun_on_crate(self, dumps):
        return np.array([on_crate(self.c, dumps.states[e], dumps.tiles[e]) for e in range(dumps.states.shape[0])])

    def coinrun_progress(self, dumps):
        """agent_x / coin_x, the coin being the row's last record."""
        c, st = self.c, dumps.states
        last = c.fixed + (st[:, c.f["n_things"]].astype(int) - 1) * c.record + c.r["x"]
        return st[:, c.f["agent_x"]] / st[np.arange(st.shape[0]), last]

    def coinrun_lava_near(self, dumps, within=8):
        """The envs with a lava tile within `within` columns of the agent's."""
        c = self.c
        lava = np.isin(dumps.tiles.reshape(-1, c.tile_w, c.tile_h), CR_LAVA).any(axis=2)  # [env, x]
        x = np.floor(dumps.states[:, c.f["agent_x"]]).astype(int)
        return np.array([lava[e, max(0, x[e] - within):x[e] + within + 1].any() for e in range(x.size)])

    def coinrun_hazard_in_view(self, dumps, within=6):
        """The envs with a lava tile or a saw (a hazard record that does not walk) within `within` cells of the agent both
        ways: a frame shows 13.3 cells across, the agent in the middle."""
        c, st = self.c, dumps.states
        out = np.zeros(st.shape[0], bool)
        for e in range(st.shape[0]):
            ax, ay = float(st[e, c.f["agent_x"]]), float(st[e, c.f["agent_y"]]) - 0.5
            x, row = int(math.floor(ax)), int(math.floor(ay))
            grid = dumps.tiles[e].reshape(c.tile_w, c.tile_h)[max(0, x - within):x + within + 1, max(0, c.tile_h - 1 - row - within):c.tile_h - row + within]
            rec = c.records(st[e])[:-1]
            saws = rec[rec[:, c.r["vel_x"]] == 0]
            out[e] = np.isin(grid, CR_LAVA).any() or ((np.abs(saws[:, c.r["x"]] - ax) <= within) & (np.abs(saws[:, c.r["y"]] - ay) <= within)).any()
        return out

    def coinrun_death(self, st, tiles):
        """What a terminal coinrun row died of: 'lava' with a lava tile under the body, else 'mob' or 'saw' by the first
        hazard record (every record but the coin's; a mob's walks) whose box the body touches, else 'other'."""
        c = self.c
        ax, ay = float(st[c.f["agent_x"]]), float(st[c.f["agent_y"]])
        x0, x1, y0, y1 = ax - 0.5, ax + 0.5, ay - 1.0, ay
        for x in range(int(math.floor(x0)), int(math.ceil(x1))):
            for row in range(int(math.floor(y0)), int(math.ceil(y1))):
                if _cr_tile(tiles, c.tile_w, c.tile_h, x, row) in CR_LAVA:
                    return "lava"
        for rec in c.records(st)[:-1]:
            mob = rec[c.r["vel_x"]] != 0
            hx, hy, hw, hh = (rec[c.r["x"]] - 0.5, rec[c.r["y"]] - 0.48, 1.0, 0.98) if mob else (rec[c.r["x"]] - 0.5, rec[c.r["y"]] - 0.5, 1.0, 1.0)
            if x0 < hx + hw and x1 > hx and y0 < hy + hh and y1 > hy:
                return "mob" if mob else "saw"
        return "other"

    def _rare_in_order(self, groups, turning):
        """At most RARE_ENVS envs: the groups' in the order given, then `turning`'s, another of them first in every step."""
        order = [np.nonzero(x)[0] for x in groups] + [np.roll(np.nonzero(turning)[0], -self.turns)]
        order = np.concatenate(order)
        rare = np.zeros(turning.size, bool)
        rare[order[np.sort(np.unique(order, return_index=True)[1])][:RARE_ENVS]] = True
        self.turns += 1
        return rare

    def caveflyer_targets(self, dumps):
        rec = self._records(dumps)
        return ((rec[:, :, self.c.r["alive"]] != 0) & (rec[:, :, self.c.r["kind"]] == TARGET)).sum(axis=1)

    def caveflyer_overflow(self, dumps):
        """The envs whose puffs, live sprites, bullets and ship are more than a wavefront has lanes."""
        c = self.c
        sprites = (self._records(dumps)[:, :, c.r["alive"]] != 0).sum(axis=1)
        return cave_draws(c, sprites, dumps.states[:, c.f["s_count"]].astype(int)) > LANES

    def _records(self, dumps):
        c = self.c
        return dumps.states[:, c.fixed:].reshape(dumps.states.shape[0], -1, c.record)  # (zeros behind an env's last record)

    def climber_coins(self, dumps):
        rec = self._records(dumps)
        return ((rec[:, :, self.c.r["alive"]] != 0) & (rec[:, :, self.c.r["vel_x"]] == 0)).sum(axis=1)

    def chaser_food(self, dumps):
        rec = self._records(dumps)
        return ((rec[:, :, self.c.r["alive"]] != 0) & (rec[:, :, self.c.r["kind"]] != EGG)).sum(axis=1)

    def step(self, before, after, reward, done, actions=None):
        """actions: the step's (caveflyer's full ring is counted after a step that fired)."""
        c, k, f, r = self.c, self.counts, self.c.f, self.c.r
        n = done.size
        starts = np.ones(n, bool) if self.first else self.resetting  # the envs whose level begins: in `before` at first, then in `after`
        level = before if self.first else after
        self.first = False
        playing = ~self.resetting
        ended = (done != 0) & playing
        win = ended & ((reward > 0) if self.game == "bossfight" else (reward >= 10))
        death = ended & ~win
        k["wins"] += int(win.sum())
        k["deaths"] += int(death.sum())
        k["ends"] += int(ended.sum())
        rare = np.zeros(n, bool)
        if self.game == "bossfight":
            k["win_and_death_steps"] += int(win.any() and (ended & (reward < 0)).any())
            phase, hp, booms = (after.states[:, f[name]].astype(int) for name in ("phase_index", "hp", "x_count"))
            k["phases"] |= set(phase[playing].tolist())
            k["damaged"] += int((playing & (hp == 0) & (booms > 0)).sum())
            rare = playing & ((phase % 2 == 1) | (hp == 0) | (booms > 0) | (phase >= 4))
        elif self.game == "climber":
            k["rewards_11"] += int((ended & (reward >= 11)).sum())
            had, has = self.climber_coins(before), self.climber_coins(after)
            self.level_coins[starts] = self.climber_coins(level)[starts]
            lost = playing & (has < had)
            k["coins"] += int((had - has)[playing].sum())
            assert not has[win].any()
            k["wins_with_3_coins"] += int((self.level_coins[win] >= 3).sum())
            k["most_coins_in_a_win"] = max([k["most_coins_in_a_win"]] + self.level_coins[win].tolist())
            rare = lost | (self.lost_coin & playing)  # a coin just destroyed, and the step after
            self.lost_coin = lost
        elif self.game == "chaser":
            self.board[starts] = self.chaser_food(level)[starts]
            self.ate_85[starts] = False
            share = 1.0 - self.chaser_food(after) / self.board.astype(float)
            k["best_share"] = max(k["best_share"], float(share[playing].max()) if playing.any() else 0.0)
            crossed = playing & (share >= 0.85) & ~self.ate_85  # (once an episode)
            self.ate_85 |= crossed
            k["wins_or_85"] += int(crossed.sum())
            b, a = self._records(before), self._records(after)
            back = ((b[:, :, r["kind"]] == EGG) & (b[:, :, r["alive"]] != 0) & (b[:, :, r["hatch_timer"]] >= HATCH_TIME)
                    & (a[:, :, r["hatch_timer"]] < 1.0)).sum(axis=1)
            back[~playing | (before.states[:, f["eat_timer"]] <= 0)] = 0
            k["eaten_enemies"] += int(back.sum())
            rare = (back > 0) & (after.states[:, f["eat_timer"]] > 0)
        elif self.game == "caveflyer":
            shots = after.states[:, f["s_count"]].astype(int)
            targets = reward - np.where(reward >= 10, 10, 0)  # 3.0 a target, beside the goal's 10.0
            hit = playing & (targets >= 3)
            full = playing & (shots == len(c.slots("shot", "frame")))
            over = playing & self.caveflyer_overflow(after)
            k["target_steps"] += int(hit.sum())
            k["double_target_steps"] += int((hit & (reward >= 6) & (reward < 10)).sum())
            k["goal_with_target_steps"] += int((hit & (reward >= 13)).sum())
            k["most_shots"] = max(k["most_shots"], int(shots[playing].max()) if playing.any() else 0)
            for least in (8, 16, 24):
                k["steps_over_%d" % least] += int((playing & (shots > least)).sum())
            k["ring_full_steps"] += int((full & (np.asarray(actions) == FIRE)).sum())
            k["overflow_steps"] += int(over.sum())
            k["most_turn"] = max(k["most_turn"], float(np.abs(after.states[playing, f["agent_rot"]]).max()) if playing.any() else 0.0)
            # (a step's reward is its last sub-step's: a target destroyed in one of the first three pays nothing)
            lost = playing & (self.caveflyer_targets(after) < self.caveflyer_targets(before))
            k["targets_destroyed"] += int((self.caveflyer_targets(before) - self.caveflyer_targets(after))[lost].sum())
            # the rarest first: a target destroyed in this step and the step after, a full ring, more draws than lanes, then
            # the envs with more than two gangs of bullets, another of them first in every step
            order = [np.nonzero(x)[0] for x in (hit | lost | (self.hit_target & playing), full, over, playing & (shots > 16))]
            order = np.concatenate(order[:3] + [np.roll(order[3], -self.turns)])
            rare[order[np.sort(np.unique(order, return_index=True)[1])][:RARE_ENVS]] = True
            self.hit_target = hit | lost
            self.turns += 1
        if self.game in ("coinrun", "jumper", "maze"):
            self.env_ends[ended] += 1
            k["most_ends"] = int(self.env_ends.max())
            least = 5 if self.game == "maze" else 3
            deep = starts & (self.env_ends >= least) & (level is after)  # the first step of a level this deep in the env's chain
            k["deep_starts"] += int(deep.sum())
        if self.game == "coinrun":
            k["envs_with_3_ends"] = int((self.env_ends >= 3).sum())
            for e in np.nonzero(death)[0]:
                k[self.coinrun_death(after.states[e], after.tiles[e]) + "_deaths"] += 1
            share = self.coinrun_progress(after)
            stood, stands = self.coinrun_on_crate(before) & playing, self.coinrun_on_crate(after) & playing
            drop = stood & np.isin(np.asarray(actions), (0, 3, 6)) & (after.states[:, f["agent_y"]] > before.states[:, f["agent_y"]]) & ~ended
            k["env_steps"] += int(playing.sum())
            k["past_half"] += int((playing & (share > 0.5)).sum())
            k["past_09"] += int((playing & (share > 0.9)).sum())
            k["crate_steps"] += int(stands.sum())
            k["drop_steps"] += int(drop.sum())
            rare = self._rare_in_order((deep, drop | (self.dropped & playing), stands, playing & (share > 0.9)), playing & self.coinrun_lava_near(after))
            self.dropped = drop
        elif self.game == "jumper":
            none_left = playing & (after.states[:, f["agent_jumps"]] == 0)
            timed = none_left & (after.states[:, f["agent_jump_timer"]] > 0)
            k["no_jump_steps"] += int(none_left.sum())
            k["no_jump_timer_steps"] += int(timed.sum())
            at = after.states[:, [f["agent_x"], f["agent_y"]]].astype(float)
            self.began_at[starts] = level.states[:, [f["agent_x"], f["agent_y"]]][starts]
            self.far_from_start = far = np.where(playing, np.hypot(*(at - self.began_at).T), 0.0)
            groups = [deep]
            if self.mode == MEMORY:
                k["farthest"] = max(k["farthest"], float(far[playing].max()) if playing.any() else 0.0)
                angle = np.arctan2(after.states[playing, f["to_goal_y"]].astype(float), after.states[playing, f["to_goal_x"]].astype(float))
                octant = np.minimum(7, np.floor((angle + math.pi) / (0.25 * math.pi)).astype(int))
                k["octants"] |= set(octant.tolist())
                self.env_octants[np.nonzero(playing)[0], octant] = True
                k["most_octants_in_an_env"] = int(self.env_octants.sum(axis=1).max())
                groups.append(playing & (far > 15))
            k["envs_with_no_end"] = int((self.env_ends == 0).sum())
            rare = self._rare_in_order(groups, timed)
        elif self.game == "maze":
            self.length[playing] += 1
            k["longest_episode"] = max([k["longest_episode"]] + self.length[ended].tolist())
            self.length[ended] = 0
            k["median_ends"] = float(np.median(self.env_ends))
            rare = deep
        self.rare = [int(e) for e in np.nonzero(rare)[0][:RARE_ENVS]]
        self.after = after
        self.resetting = done != 0


def run_on_oracle(game, mode, each_step=None, at_start=None, render=False, threads=1, n=N, steps=None, ora=None, actions_of=None):
    """The lock-step protocol on an OracleVec.  at_start(ora) before the first step; each_step(s, ora, actions, obs, reward,
    done, counter) after every step, counter.rare naming the envs in a rare state.  Returns the counts.  `ora`: an oracle
    the caller made (and closes); actions_of(step, n): other actions than the agents' (the census of random play)."""
    from oracle_util import OracleVec
    own = ora is None
    if own:
        ora = OracleVec(game, n, seed_base=SEED_BASE, render=render, mode=mode, threads=threads)
    c, counter, rng = columns(game, mode), Counter(game, mode, n), np.random.default_rng(POLICY_SEED)
    try:
        if at_start:
            at_start(ora)
        before = Dumps(ora, c)
        for s in range(STEPS[(game, mode)] if steps is None else steps):
            a = choose_actions(game, mode, before, s, rng) if actions_of is None else actions_of(s, n)
            obs, reward, done = ora.step(a, threads=threads)
            after = Dumps(ora, c)
            counter.step(before, after, reward, done, a)
            if each_step:
                each_step(s, ora, a, obs, reward, done, counter)
            before = after
    finally:
        if own:
            ora.close()
    return counter.counts


RARE_FLOOR = 20  # the GPU half compares state and tile rows in at least this many envs a case
COMPASS = set(range(8))  # jumper's memory mode: the octants of atan2(to_goal_y, to_goal_x)
# maze: the episodes the median env of this protocol ends under random play (tests/variant_paths_util.py's actions), by mode:
# (in STEPS steps, in that protocol's own 520); tests/test_scripted_play.py holds the figures to a run.  Twice the first asks
# for nothing, so the floor is twice the larger of the two: what random play needs the 500-step cap and more for
RANDOM_MAZE_MEDIAN = {EASY: (0, 1), HARD: (0, 1), MEMORY: (0, 1)}
# jumper's memory mode: the compass's octants met inside ONE env — more than half the compass, so an agent that went round its
# goal.  (All eight are met at step 0 already when 65 envs are counted together, under any play.)
OCTANTS_IN_AN_ENV = 5


def floors(game, mode):
    """count name → the least a run must reach."""
    if game == "bossfight":
        return dict(wins=5, deaths=5, damaged=50, win_and_death_steps=1)
    if game == "climber":
        return dict(wins=5, wins_with_3_coins=1, rewards_11=1, coins=40, deaths=3)
    if game == "caveflyer":
        out = dict(wins=5, deaths=3, target_steps=5, steps_over_8=100, steps_over_16=20)
        out.update(dict(ring_full_steps=1, overflow_steps=20) if mode == MEMORY else dict(most_shots=20))
        return out
    if game == "coinrun":
        return dict(wins=100, deaths=30, lava_deaths=5, saw_deaths=5, mob_deaths=5, envs_with_3_ends=60, most_ends=8, crate_steps=20, drop_steps=5,
                    deep_starts=RARE_FLOOR)
    if game == "jumper":
        out = dict(wins={EASY: 100, HARD: 40, MEMORY: 40}[mode], most_ends={EASY: 8, HARD: 6, MEMORY: 3}[mode], no_jump_steps=5000,
                   no_jump_timer_steps=RARE_FLOOR)
        out.update(dict(farthest=20, most_octants_in_an_env=OCTANTS_IN_AN_ENV) if mode == MEMORY else dict(deaths=20))
        return out
    if game == "maze":
        return dict(wins=100, median_ends=2 * max(RANDOM_MAZE_MEDIAN[mode]), deep_starts=RARE_FLOOR)
    out = dict(eaten_enemies=20, deaths=3)
    out["wins_or_85" if (game, mode) in ATE_85_INSTEAD else "wins"] = 2 if mode == EASY else 1
    return out


def assert_covers(game, mode, counts):
    for name, least in floors(game, mode).items():
        assert counts[name] >= least, "%s mode %d: %s is %d, the floor is %d (%r)" % (game, mode, name, counts[name], least, counts)
    if game == "bossfight":
        assert counts["phases"] >= set(range(6)), "%s mode %d: phases seen %r" % (game, mode, sorted(counts["phases"]))
    if game == "coinrun":
        for name, share in (("past_half", 0.25), ("past_09", 0.05)):
            assert counts[name] >= share * counts["env_steps"], "%s mode %d: %s is %d of %d env-steps" % (game, mode, name, counts[name], counts["env_steps"])
    if (game, mode) == ("jumper", MEMORY):
        assert counts["deaths"] == 0, "jumper's memory mode has no spikes: %r" % counts
        assert counts["octants"] == COMPASS, "jumper mode %d: the compass pointed into octants %r" % (mode, sorted(counts["octants"]))
    if game == "caveflyer":
        assert counts["most_turn"] > FULL_TURN, "%s mode %d: the ship turned %.3f at the most" % (game, mode, counts["most_turn"])


# test_same_step_episodes_of_scripted_play (tests/test_scripted_play_gpu.py): the agents on the model of tests/episodes_util.py,
# same-step auto-reset, no limit, a ring of 4 terminal frames, each game in its default mode, seed_base 1 as the model's
SAME_STEP_RING, SAME_STEP_WINS = 4, 1
DEFAULT_MODE = {g: TABLE[g][0] for g in GAMES}


def run_same_step(game, model, eng=None, check_step=None, steps=None):
    """The agents play on `model` (an EpisodeModel in same-step mode, after its first reset), reading the model's own oracle
    (model.o: after a step it already shows the next level of an env that ended); an engine beside it gets the same actions
    and check_step(eng, model, got, t) holds it to the model.  Returns the counts."""
    mode = DEFAULT_MODE[game]
    c, rng = columns(game, mode), np.random.default_rng(POLICY_SEED)
    k = dict(ends=0, wins=0, wins_with_frame=0, longest_win=0, best_return=0.0)
    for t in range(STEPS[(game, mode)] if steps is None else steps):
        a = choose_actions(game, mode, Dumps(model.o, c), t, rng)
        got = eng.step(a) if eng is not None else None
        model.step(a)
        if eng is not None:
            check_step(eng, model, got, t)
        won = model.reward[model.ended_env] > 0 if game == "bossfight" else model.reward[model.ended_env] >= 10
        k["ends"] += int(model.counts[0])
        k["wins"] += int(won.sum())
        k["wins_with_frame"] += int(won[:model.counts[1]].sum())
        if won.any():
            k["longest_win"] = max(k["longest_win"], int(model.ended_length[won].max()))
            k["best_return"] = max(k["best_return"], float(model.ended_return[won].max()))
    return k


def assert_same_step_covers(game, counts):
    assert counts["wins_with_frame"] >= SAME_STEP_WINS, "%s: %r" % (game, counts)
