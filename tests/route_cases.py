"""What tests/test_route.py (CPU) and tests/test_gpu_route*.py (engine states)
share: the goals drawn for the goal column, and the hand-built serpentine.
"""
import numpy as np

GROUND, WALL, STAIR = 1, 2, 3
GOAL_CLASSES = ("ground", "unknown", "wall", "none")


def draw_goals(rs, tiles, known, H):
    """``(goal, classes)``: int32 [B], per game a known Ground cell, an unknown
    cell, a Wall cell or -1, and the class each game got (``none`` where the
    game has no cell of the class drawn).  ``tiles`` int [B, W, H], ``known``
    bool [B, W, H]."""
    B = len(tiles)
    goal, classes = np.full(B, -1, np.int32), []
    for i in range(B):
        cls = GOAL_CLASSES[rs.randint(4)]
        pick = {"ground": known[i] & (tiles[i] == GROUND), "unknown": ~known[i],
                "wall": tiles[i] == WALL, "none": np.zeros_like(known[i])}[cls]
        at = np.argwhere(pick)
        if len(at):
            x, y = at[rs.randint(len(at))]
            goal[i] = x * H + y
        else:
            cls = "none"
        classes.append(cls)
    return goal, classes


def serpentine(W, H):
    """``(layout, start, end, moves)``: a one-wide corridor through a W x H grid
    of Wall (W, H even) -- along every odd row from x = 1 to x = W - 2, joined to
    the next odd row at alternating ends -- from ``start`` = (1, 1) to the
    StaircaseDown ``end``, and the number of moves between them, from the
    construction: ``rows`` runs of W - 3 moves and two moves per joint."""
    lay = np.full((W, H), WALL, np.uint8)
    rows = (H - 2) // 2                       # y = 1, 3, .., H - 3
    for r in range(rows):
        y = 2 * r + 1
        lay[1:W - 1, y] = GROUND
        if r + 1 < rows:
            lay[W - 2 if r % 2 == 0 else 1, y + 1] = GROUND
    end = (W - 2 if rows % 2 == 1 else 1, 2 * (rows - 1) + 1)
    lay[end] = STAIR
    return lay, (1, 1), end, rows * (W - 3) + (rows - 1) * 2
