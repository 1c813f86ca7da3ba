"""A third, deliberately naive statement of both games' rules (plain Python, CPU only).

The oracle (oracle/bgs_oracle.c) and the kernels share one reading of the rules that the reference does not pin
("Unpinned").  This module restates them from the rules as DESIGN.md §2 and the golden fixtures state them,
for readability and not for speed: boards are lists of rows (row 0 = bottom, the reference layout), wins are found by
walking the four directions cell by cell, and the Bounce target search is a plain recursion over (cell, steps left, last
direction).  It imports nothing from oracle/ or from the package.

Status codes follow the library: 0 = applied (or skipped), -2 = illegal, board untouched.  Winner codes: -1 running,
0 / 1 that player won, 2 draw.
"""

OK = 0
ILLEGAL = -2
RUNNING, DRAW = -1, 2


def reward(winner):
    """[player 0, player 1]: +1 / -1 for a win, 0 / 0 for a draw or a game still running"""
    if winner == 0:
        return [1, -1]
    if winner == 1:
        return [-1, 1]
    return [0, 0]


# ------------------------------------------------------------------------------------------------ Connect
# grid[y][x]: -1 empty, 0 / 1 a stone of that player; stones fall to the lowest empty cell of their column.


class Connect:
    def __init__(self, height, width, count):
        self.h, self.w, self.k = height, width, count

    def initial(self):
        return [[-1] * self.w for _ in range(self.h)], 0, RUNNING, 0

    def legal(self, grid, winner):
        """the columns a stone may be dropped in, ascending; none once the game has ended"""
        if winner != RUNNING:
            return []
        return [x for x in range(self.w) if any(grid[y][x] == -1 for y in range(self.h))]

    def _stones_in_a_row(self, grid, x, y, dx, dy):
        who = grid[y][x]
        count = 1
        for sign in (1, -1):
            cx, cy = x + sign * dx, y + sign * dy
            while 0 <= cx < self.w and 0 <= cy < self.h and grid[cy][cx] == who:
                count += 1
                cx, cy = cx + sign * dx, cy + sign * dy
        return count

    def step(self, grid, player, winner, plies, column):
        """(status, grid, player, winner, plies) after dropping a stone in `column`; a negative column skips the board"""
        grid = [row[:] for row in grid]
        if column < 0:
            return OK, grid, player, winner, plies
        if winner != RUNNING or column >= self.w or column not in self.legal(grid, winner):
            return ILLEGAL, grid, player, winner, plies
        y = 0
        while grid[y][column] != -1:
            y += 1
        grid[y][column] = player
        if any(self._stones_in_a_row(grid, column, y, dx, dy) >= self.k for dx, dy in ((1, 0), (0, 1), (1, 1), (1, -1))):
            winner = player
        elif all(grid[yy][xx] != -1 for yy in range(self.h) for xx in range(self.w)):
            winner = DRAW
        return OK, grid, 1 - player, winner, plies + 1


# ------------------------------------------------------------------------------------------------ Bounce
# grid[y][x]: 0 empty, v > 0 a piece that moves exactly v unit steps.  Rows 0 and H-1 are the goal rows: player 0 moves
# up (+y) towards row H-1, player 1 down towards row 0.  Pieces belong to nobody: a player moves a piece of the ACTIVE
# row, the non-empty row between the goal rows nearest to their own side.
#
# A move is a path of unit steps, each forward, left or right, never backward, never right straight after left or left
# straight after right.  A segment of v steps crosses only empty cells outside the goal rows; its last step lands on an
# empty cell (a target), on the mover's own goal row (a target; the opponent's goal row is closed), or on a piece, which
# starts a fresh segment of that piece's value in any direction.  The moving piece still stands on its origin while it
# moves, so a path that comes back to it bounces off it.

FORWARD, LEFT, RIGHT = "forward", "left", "right"


class Bounce:
    def __init__(self, config_grid):
        self.config = [list(map(int, row)) for row in config_grid]
        self.h, self.w = len(self.config), len(self.config[0])

    def initial(self):
        """the config grid, player 0 to move; a start without any move for player 0 is already settled: player 1 wins if
        they could move, otherwise a draw"""
        grid = [row[:] for row in self.config]
        winner = RUNNING
        if not self.actions(grid, 0, RUNNING):
            winner = 1 if self.actions(grid, 1, RUNNING) else DRAW
        return grid, 0, winner, 0

    def active_row(self, grid, player):
        rows = range(1, self.h - 1) if player == 0 else range(self.h - 2, 0, -1)
        for y in rows:
            if any(grid[y][x] > 0 for x in range(self.w)):
                return y
        return None

    def targets(self, grid, player, winner, sx, sy):
        """the set of cells (x, y) the piece on (sx, sy) may land on; empty when it is not a piece of the active row"""
        if winner != RUNNING or not (0 <= sx < self.w and 0 <= sy < self.h):
            return set()
        if grid[sy][sx] <= 0 or sy != self.active_row(grid, player):
            return set()
        forward = 1 if player == 0 else -1
        own_goal = self.h - 1 if player == 0 else 0
        found, seen = set(), set()

        def walk(x, y, steps_left, last):
            if (x, y, steps_left, last) in seen:
                return
            seen.add((x, y, steps_left, last))
            for d in (FORWARD, LEFT, RIGHT):
                if (d, last) in ((LEFT, RIGHT), (RIGHT, LEFT)):
                    continue
                nx = x + (1 if d == RIGHT else -1 if d == LEFT else 0)
                ny = y + (forward if d == FORWARD else 0)
                if not (0 <= nx < self.w and 0 <= ny < self.h):
                    continue
                goal = ny in (0, self.h - 1)
                if steps_left > 1:
                    if not goal and grid[ny][nx] == 0:
                        walk(nx, ny, steps_left - 1, d)
                elif goal:
                    if ny == own_goal:
                        found.add((nx, ny))
                elif grid[ny][nx] == 0:
                    found.add((nx, ny))
                else:
                    walk(nx, ny, grid[ny][nx], FORWARD)   # a bounce: a fresh segment, any first direction

        walk(sx, sy, grid[sy][sx], FORWARD)
        return found

    def actions(self, grid, player, winner):
        """every (source, target): sources by ascending x along the active row, targets by ascending (y, x)"""
        if winner != RUNNING:
            return []
        row = self.active_row(grid, player)
        if row is None:
            return []
        out = []
        for x in range(self.w):
            for tx, ty in sorted(self.targets(grid, player, winner, x, row), key=lambda c: (c[1], c[0])):
                out.append(((x, row), (tx, ty)))
        return out

    def step(self, grid, player, winner, plies, move):
        """(status, grid, player, winner, plies) after move = (sx, sy, tx, ty); a negative sx skips the board.  Reaching
        the goal row wins; otherwise, when the next player cannot move, the mover wins if they could move again and the
        game is drawn if not."""
        grid = [row[:] for row in grid]
        sx, sy, tx, ty = move
        if sx < 0:
            return OK, grid, player, winner, plies
        if (tx, ty) not in self.targets(grid, player, winner, sx, sy):
            return ILLEGAL, grid, player, winner, plies
        grid[ty][tx], grid[sy][sx] = grid[sy][sx], 0
        if ty in (0, self.h - 1):
            winner = player
        elif not self.actions(grid, 1 - player, RUNNING):
            winner = player if self.actions(grid, player, RUNNING) else DRAW
        return OK, grid, 1 - player, winner, plies + 1
