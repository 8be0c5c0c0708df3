"""fp64 restatement of the trajectory predictor's numbers (hideandseek.py:831-854 + TP_net, mappo.py:572-589), from fp32 inputs.
TEST REFERENCE ONLY: the yardstick of `tests/test_tp_accuracy.py`.

Input is the fp32 window the predictor ran on (`history` [U,T,I]: the device window is bit-exact with the oracle's) and the fp32
parameters; everything after that is float64: the LSTM from zero state (gate order i, f, g, o), the output layer, tanh, the rescale to
arena units, and `drone - pred` for the rpos_pred columns of `obs_self` / `state_drones`.  One evader: unit e, rows of 20 + 3F values
with the predictions in columns 3 .. 3 + 3F.  Two evaders: unit 2 e + j, rows of 24 + 6F values with evader 0's predictions in columns
3 .. 3 + 3F and evader 1's in 24 + 3F .. 24 + 6F."""
import numpy as np

WEIGHT_FIELDS = ("w_ih", "w_hh", "b_ih", "b_hh", "w_fc", "b_fc")


def lstm_fc_tanh(history, w):
    """tanh(W_fc h_T + b_fc) in float64: history [U,T,I] fp32, w {w_ih, w_hh, b_ih, b_hh, w_fc, b_fc} fp32 -> [U, 3F]."""
    X = np.asarray(history, np.float32).astype(np.float64)
    Wih, Whh = (np.asarray(w[k], np.float32).astype(np.float64) for k in ("w_ih", "w_hh"))
    b = np.asarray(w["b_ih"], np.float32).astype(np.float64) + np.asarray(w["b_hh"], np.float32).astype(np.float64)
    Wfc, bfc = (np.asarray(w[k], np.float32).astype(np.float64) for k in ("w_fc", "b_fc"))
    H = Whh.shape[1]
    U, T, _ = X.shape
    h, c = np.zeros((U, H)), np.zeros((U, H))
    for t in range(T):
        z = X[:, t] @ Wih.T + h @ Whh.T + b
        i, f, g, o = _sigmoid(z[:, :H]), _sigmoid(z[:, H:2 * H]), np.tanh(z[:, 2 * H:3 * H]), _sigmoid(z[:, 3 * H:])
        c = f * c + i * g
        h = o * np.tanh(c)
    return np.tanh(h @ Wfc.T + bfc)


def _sigmoid(z):
    return 0.5 * (1.0 + np.tanh(0.5 * z))          # no overflow of exp(-z) for large |z|


def rescale(v, arena_size, max_height):
    """hideandseek.py:835-836 in float64: x, y scaled by arena_size / 2, z mapped from [-1, 1] to [0, max_height].  v [U, 3F] -> [U, F, 3]."""
    p = np.asarray(v, np.float64).reshape(v.shape[0], -1, 3).copy()
    p[..., :2] = p[..., :2] * 0.5 * float(arena_size)
    p[..., 2] = (p[..., 2] + 1.0) * 0.5 * float(max_height)
    return p


def pred_columns(F, NT=1):
    """Columns of an `obs_self` / `state_drones` row that hold rpos_pred (drone - prediction), per evader."""
    R = 3 * F
    return [np.arange(3, 3 + R)] + ([np.arange(24 + R, 24 + 2 * R)] if NT == 2 else [])


def rpos_pred(pred, drone_pos, NT=1):
    """drone - prediction in float64 for every pursuer: pred [E*NT, F, 3], drone_pos [E,A,3] fp32 -> [NT, E, A, 3F]."""
    pred = np.asarray(pred, np.float64)
    E, A = drone_pos.shape[:2]
    pr = pred.reshape(E, NT, -1)                                            # unit 2 e + j with two evaders
    d = np.asarray(drone_pos, np.float32).astype(np.float64)
    F = pr.shape[-1] // 3
    return np.stack([(d[:, :, None, :] - pr[:, None, j].reshape(E, 1, F, 3)).reshape(E, A, 3 * F) for j in range(NT)])


def predict(history, w, arena_size, max_height, drone_pos, NT=1):
    """Everything the accuracy gate looks at: {"pred": [U,F,3], "rpos": [NT,E,A,3F]} in float64."""
    pred = rescale(lstm_fc_tanh(history, w), arena_size, max_height)
    return {"pred": pred, "rpos": rpos_pred(pred, drone_pos, NT)}


def row_rpos(rows, F, NT=1):
    """The rpos_pred columns of fp32 rows [E,A,D] as [NT,E,A,3F] (the layout `rpos_pred` returns)."""
    return np.stack([np.asarray(rows)[..., cols] for cols in pred_columns(F, NT)])


def other_columns(D, F, NT=1):
    """Columns of a row that are NOT predictions (copied or subtracted in fp32: bit-exact with the oracle)."""
    mask = np.ones(D, bool)
    for cols in pred_columns(F, NT):
        mask[cols] = False
    return np.nonzero(mask)[0]
