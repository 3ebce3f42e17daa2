"""Host mirror of the reference's LDP predictor daemon
(/root/reference/HM-16.5_Test_LDP/bin/resi_to_cu_depth_LDP.py): same files, same handshake, so
the unchanged HM-LDP encoder (TEncGOP.cpp:1463-1503) drives it:

    HM:     pre-encode -> resi.yuv ; command.dat = "<POC> <w> <h> <qp> [end]" ; touch pred_start.sig
    daemon: read command, remove pred_start.sig, (re)load the LSTM model when the QP changed,
            predict, write state.dat, cu_depth.dat, then touch pred_end.sig
    HM:     spin on pred_end.sig, remove it, fread cu_depth.dat (nctu x 21 float32)

Everything numeric happens in libethcnn.so (ethcnn_ldp_predict_frame: resi_cnn + one ETH-LSTM
step + heads + gates on the GPU).  Differences from the reference, none in the numbers:
  * cu_depth.dat / state.dat are written to temp files and renamed before pred_end.sig appears;
  * the poll loop sleeps 200 us between checks instead of spinning, and `serve` can stop after
    `max_frames` or an idle timeout (tests; the reference loops forever);
  * the recurrent state stays RESIDENT IN HBM between frames (ethcnn_ldp_step): only the daemon itself
    ever reads state.dat back (:103-106), so the per-frame 2 x nctu x 3.5 KB PCIe round trip is not on the
    encoder's critical path.  state.dat is still written every frame for protocol compatibility -- AFTER
    cu_depth.dat and pred_end.sig, while HM is already encoding -- and it is still the source whenever
    the resident state cannot be the right one (daemon restart, a frame out of sequence, a state.dat
    somebody else replaced: inode / size / mtime are checked).  A sidecar `state.dat.idx` brackets the late write:
    "pending <i_frame> <w> <h>" appears BEFORE pred_end.sig, "<i_frame> <w> <h>" replaces it once state.dat holds that
    frame's state.  A restarted daemon that finds "pending" (the previous daemon died between the ending signal and the
    state write, so state.dat still belongs to an earlier frame) refuses the file instead of silently feeding a stale
    state into the recurrence; a state.dat without sidecar (the reference daemon's) is taken as it is, whatever frame
    it is from -- as the reference does (HM may skip frames: intra pictures are not predicted);
  * resi.yuv is read straight into pinned host memory (DMA-able without a staging copy);
  * missing trained CNN blob (model_LDP_2000000_qp22~37.dat.data is not in the reference repo):
    ETHCNN_SYNTHETIC_SEED=<n> opts into seeded synthetic CNN weights, otherwise it is an error;
  * ETHCNN_SEARCH_BUDGET=<share, 0..1> [ETHCNN_SEARCH_BUDGET_MODE=frame|carry] [ETHCNN_SEARCH_BUDGET_WEIGHTS="64 16 4 1"] holds every
    frame's pruned search under that share of the full search's weighted checks (include/ethcnn.h "search budget, online"): the daemon
    predicts with open gates, whatever Thr_info.txt says, and a pacer (ethcnn.Pacer) picks a rung of the default ladder (or of the
    ladder file ETHCNN_SEARCH_BUDGET_LADDER, in Low-Delay-P token order: tools/build_ladder.py --out FILE --order ldp) per frame and
    bakes the picked decisions into cu_depth.dat (values 0, 0.5, 1) inside the handshake.  The encoder reads Thr_info.txt itself, so the
    daemon refuses at start-up (status 1, before a GPU is touched, no signal file) unless that file is the companion line in
    Low-Delay-P token order, "0.25 0.75 0.25 0.75 0.25 0.75".  A frame with i_frame <= 1 or another geometry starts a new allowance.
    ETHCNN_SEARCH_BUDGET_LADDER=auto, which lets the All-Intra launcher build the ladder from the sequence it predicts, is refused at
    start-up with the reason: this loop sees one frame at a time.
  * --sessions DIR [DIR ...] serves several working directories from one context (serve_many); there the budget is given on the command
    line, --budget SHARE [--budget-mode frame|carry] [--budget-weights "64 16 4 1"] [--budget-ladder FILE], under the value rules above,
    and is held for every directory by ONE pacer set (ethcnn.PacerSet): a directory's session is its slot, a round of directories is one
    call behind the round's step.  The environment variables stay refused under --sessions.
  * --sessions ... --budget-policies FILE gives every directory a policy of its own; the --budget options, if any, are the default
    policy.  One policy per line, `#` starts a comment: SELECTOR SHARE [MODE [LADDER|- [W64 W32 W16 W8]]] with SELECTOR dir=PATH,
    qp=LO..HI (inclusive) or *; ladder files in Low-Delay-P token order, `-` the default ladder.  Where a directory's slot would be reset
    (i_frame <= 1 or another picture size) it is bound instead: to the first dir= line whose realpath is the directory's, else the first
    qp= line that holds the QP of that frame, else the first *, else --budget.  The binding holds until the next start.  Refused at
    start-up (status 1, nothing written, no GPU touched): what check_policies lists.
"""
from __future__ import print_function

import os
import sys
import time

import numpy as np

from . import ethcnn as _e
from . import net_CNN as nt
from . import search_budget as _sb

# ETHCNN_SEARCH_BUDGET_LADDER=auto builds a ladder from the predictions of the whole sequence; this daemon predicts frame by frame
NO_AUTO_LADDER = ('the Low-Delay-P loop predicts one frame at a time and cannot see the sequence in advance; build the ladder offline '
                  '(tools/build_ladder.py --no-labels --out FILE --order ldp) and name the file')
IMAGE_SIZE = nt.IMAGE_SIZE
NUM_CHANNELS = nt.NUM_CHANNELS
NUM_EXT_FEATURES = 2      # QP and POC (resi_to_cu_depth_LDP.py:19)
VECTOR_LENGTH = _e.NVEC   # config.py VECTOR_LENGTH = 64 + 128 + 256
LSTM_MAX_LENGTH = 1
LSTM_DEPTH = 1
MINI_BATCH_SIZE = 1024    # :118 (gate scope; applied inside the library)

COMPLETE_FILE = 'complete.dat'
YUV_FILE = 'resi.yuv'
STATE_FILE = 'state.dat'
STATE_INDEX_SUFFIX = '.idx'   # ours: "[pending] <i_frame> <w> <h>": the frame whose output state state.dat holds / is about to hold
SAVE_FILE = 'cu_depth.dat'
COMMAND_FILE = 'command.dat'
START_FILE = 'pred_start.sig'
END_FILE = 'pred_end.sig'
THR_FILE = 'Thr_info.txt'
MODEL_CNN_FILE = 'model_LDP_2000000_qp22~37.dat'  # :159


class StaleStateError(IOError):
    """state.dat cannot be the state of the previous frame (see get_state_in_from_one_file)."""


def send_init_signal(init_file):
    with open(init_file, 'w+') as f:
        f.write('1')
    print('Python: predictor initialized.')


def send_complete_signal(complete_file):
    with open(complete_file, 'w+') as f:
        f.write('1')
    print('Python: Operation completed.')


def get_command(command_file):
    """:56-72: '<i_frame> <w> <h> <qp> [end]' -> ints, or four -1 while the line is incomplete."""
    try:
        with open(command_file, 'r') as f:
            str_arr = f.readline().split(' ')
    except IOError:
        return -1, -1, -1, -1
    if len(str_arr) == 5 and str_arr[4] == '[end]':
        try:
            return int(str_arr[0]), int(str_arr[1]), int(str_arr[2]), int(str_arr[3])
        except ValueError:
            pass
    return -1, -1, -1, -1


def get_images_from_one_file(yuv_file, frame_width, frame_height, CUwidth=IMAGE_SIZE, into=None):
    """:74-101 reads the first frame's luma; the zero-padded 64x64 tiling happens on the GPU.
    Returns (luma [h, w] uint8, num_vectors).  `into`: a (pinned) uint8 buffer to read into."""
    assert CUwidth == IMAGE_SIZE
    want = frame_width * frame_height
    with open(yuv_file, 'rb') as f:
        if into is not None:
            got = f.readinto(memoryview(into[:want]))
            luma = into[:want]
        else:
            y_buf = f.read(want)
            got = len(y_buf)
            luma = np.frombuffer(y_buf, dtype=np.uint8)
    if got != want:
        raise IOError('%s: short read (%d of %d luma bytes)' % (yuv_file, got, want))
    return luma.reshape(frame_height, frame_width), _e.ctus_per_frame(frame_width, frame_height)


def get_state_in_from_one_file(state_file, num_vectors, i_frame, geometry=None):
    """:103-112: zeros for i_frame <= 1 (returned as None = zeros inside the library).  The sidecar this daemon writes
    must not say "pending" (the state write behind an ending signal never completed: the file is an EARLIER frame's) and
    must name `geometry` = (w, h) when given: a stale state is an error, never a silently wrong recurrence."""
    if i_frame > 1:
        try:
            with open(state_file + STATE_INDEX_SUFFIX, 'r') as f:
                tag = f.read().split()
        except (IOError, OSError):
            tag = None  # no sidecar: somebody else's state.dat (the reference daemon writes none) -> trusted as there
        if tag is not None:
            if tag[:1] == ['pending']:
                raise StaleStateError('%s is stale: the state of frame %s was never written (the daemon that served it stopped after '
                                      'its ending signal); delete %s%s to accept %s as it is, or restart the encode'
                                      % (state_file, tag[1] if len(tag) > 1 else '?', state_file, STATE_INDEX_SUFFIX, state_file))
            if len(tag) != 3 or (geometry is not None and [str(int(g)) for g in geometry] != tag[1:]):
                raise IOError('%s belongs to another sequence (%s), frame %d is %s' % (state_file, ' '.join(tag), i_frame, geometry))
        want = num_vectors * LSTM_DEPTH * 2 * VECTOR_LENGTH
        state_in = np.fromfile(state_file, dtype=np.float32, count=want)
        if state_in.size != want:
            raise IOError('%s: holds %d floats, need %d' % (state_file, state_in.size, want))
        return state_in.reshape(num_vectors, LSTM_DEPTH, 2, VECTOR_LENGTH)
    return None


def predict_cu_depth(ctx, luma, frame_width, frame_height, state_in, qp_seq, i_frame):
    """:114-129 -> (depth_out [n, 21], state_out [n, 1, 2, 448])"""
    n = _e.ctus_per_frame(frame_width, frame_height)
    sin = None if state_in is None else np.asarray(state_in, dtype=np.float32).reshape(n, 2, VECTOR_LENGTH)
    depth_out, state_out = ctx.ldp_predict_frame(luma, frame_width, frame_height, qp_seq, i_frame, sin)
    return depth_out, state_out.reshape(n, LSTM_DEPTH, 2, VECTOR_LENGTH)


def _file_sig(path):
    try:
        st = os.stat(path)
        return st.st_ino, st.st_size, st.st_mtime_ns  # inode: a same-size replacement inside one timestamp tick is still seen
    except OSError:
        return None


def _write_atomic(path, arr):
    tmp = '%s.tmp.%d' % (path, os.getpid())
    with open(tmp, 'wb') as f:
        f.write(np.ascontiguousarray(arr, dtype=np.float32).tobytes())
    os.rename(tmp, path)


def save_cu_depth(depth_out, save_file, state_file, end_file, num_vectors, tag=None):
    """The half of save_cu_depth_and_state that the encoder waits for: the "pending" sidecar (tag = (i_frame, w, h)), cu_depth.dat, the
    ending signal.  Returns the other half as a function of the state: state.dat, then the sidecar in its final form."""
    assert depth_out.size == num_vectors * (1 + 4 + 16)

    def sidecar(text):
        tmp = '%s%s.tmp.%d' % (state_file, STATE_INDEX_SUFFIX, os.getpid())
        with open(tmp, 'w') as f:
            f.write(text + '\n')
        os.rename(tmp, state_file + STATE_INDEX_SUFFIX)

    def finish(state_out):
        _write_atomic(state_file, state_out)
        if tag is not None:
            sidecar('%d %d %d' % tuple(tag))
    if tag is not None:
        sidecar('pending %d %d %d' % tuple(tag))  # from here until finish(), state.dat is an earlier frame's
    _write_atomic(save_file, depth_out)
    open(end_file, 'wb').close()
    return finish


def save_cu_depth_and_state(depth_out, state_out, save_file, state_file, end_file, num_vectors, tag=None):
    """:131-145 writes state.dat, cu_depth.dat, then the (empty) ending signal.  Here cu_depth.dat and the ending
    signal come FIRST (they are what HM waits for) and state.dat is refreshed afterwards, while HM is already
    encoding: `state_out` may be a callable that fetches the state from the GPU at that point.  Returns the state."""
    finish = save_cu_depth(depth_out, save_file, state_file, end_file, num_vectors, tag)
    if callable(state_out):
        state_out = state_out()
    finish(state_out)
    return state_out


def restore_cnn(ctx, model_dir='.'):
    prefix = os.path.join(model_dir, MODEL_CNN_FILE)
    seed = os.environ.get('ETHCNN_SYNTHETIC_SEED')
    if os.path.exists(prefix + '.data-00000-of-00001') or seed is None:
        ctx.load_checkpoint(prefix)
        return prefix
    ctx.load_synthetic(int(seed), float(os.environ.get('ETHCNN_HEAD_GAIN', '1.0')))
    return 'synthetic(seed=%s)' % seed


def restore_lstm(ctx, qp_seq, model_dir='.'):
    """:166-179: QP band -> LSTM checkpoint."""
    prefix = os.path.join(model_dir, _e.lstm_model_name_for_qp(qp_seq))
    seed = os.environ.get('ETHCNN_SYNTHETIC_SEED')
    if os.path.exists(prefix + '.data-00000-of-00001') or seed is None:
        ctx.load_lstm_checkpoint(prefix)
        return prefix
    ctx.load_lstm_synthetic(int(seed), float(os.environ.get('ETHCNN_HEAD_GAIN', '1.0')))
    return 'synthetic(seed=%s)' % seed


def serve(workdir='.', max_frames=None, idle_timeout=None, poll_s=2e-4, device=0, verbose=True, accept_stale=False):
    """The daemon loop (:148-190).  Returns the number of frames predicted.
    A stale state.dat (sidecar says "pending": the daemon that served that frame stopped between its ending signal and its
    state write) stops the daemon with StaleStateError and a message that names the recovery -- delete state.dat.idx to accept
    state.dat as it is, or restart the encode -- unless accept_stale is set, in which case the file is used as it is after
    a warning.  (HM then keeps spinning on pred_end.sig, exactly as it does when the reference's daemon dies.)"""
    p = lambda name: os.path.join(workdir, name)
    budget, ladder = _sb.from_env(), None   # (ValueError for a bad value: before a GPU is touched)
    if budget is not None:
        ladder = _sb.ladder_from_env('ldp', auto=NO_AUTO_LADDER)
        _sb.check_companion_thr_file(p(THR_FILE), _sb.COMPANION_LINE_LDP)
    ctx = _e.EthCnn(device=device)
    pacer, paced_geom, paced = None, None, [0, 0, 0, 0]   # frames, over budget, sum of cost, sum of full
    try:
        ctx.load_thresholds(p(THR_FILE))
        if budget is not None:
            ctx.set_thresholds(0.0, 0.0)    # open gates, whatever Thr_info.txt says: the baked file is what the encoder reads
            pacer = _e.Pacer(ctx, budget[0], budget[1], ladder=None if ladder is None else _e.sim_thr(*ladder), weights=budget[2])
        restore_cnn(ctx, workdir)
        if verbose:
            print('Python: predictor initialized on %s.' % ctx.device_name)
        n_frame_total, qp_seq = 0, 0
        last_key, state_sig = None, None   # (w, h, i_frame) of the resident state; (size, mtime_ns) of the state.dat we wrote
        pinned, pinned_probs = None, None  # capacities tracked separately: 65x65 has fewer pixels but more CTUs than 128x64
        idle_since = time.time()
        while max_frames is None or n_frame_total < max_frames:
            if not os.path.isfile(p(START_FILE)):
                if idle_timeout is not None and time.time() - idle_since > idle_timeout:
                    break
                time.sleep(poll_s)
                continue
            i_frame, frame_width, frame_height, qp_seq_temp = get_command(p(COMMAND_FILE))
            if i_frame < 0:
                time.sleep(poll_s)
                continue
            qp_seq_last, qp_seq = qp_seq, qp_seq_temp
            os.remove(p(START_FILE))
            if qp_seq != qp_seq_last:
                name = restore_lstm(ctx, qp_seq, workdir)
                if verbose:
                    print('Set QP = %d' % qp_seq)
                    print('LSTM model loaded (%s).' % name)
            need_px, need_pr = frame_width * frame_height, _e.ctus_per_frame(frame_width, frame_height) * 21
            if pinned is None or pinned.size < need_px or pinned_probs.size < need_pr:
                need_px = max(need_px, 0 if pinned is None else pinned.size)
                need_pr = max(need_pr, 0 if pinned_probs is None else pinned_probs.size)
                ctx.free_host_buffers()
                pinned = ctx.host_buffer(need_px)
                pinned_probs = ctx.host_buffer(need_pr * 4).view(np.float32)
            luma, num_vectors = get_images_from_one_file(p(YUV_FILE), frame_width, frame_height, IMAGE_SIZE, into=pinned)
            # the state of frame i_frame - 1 is resident in HBM when this daemon produced it for this geometry and the
            # state.dat it wrote then is still the one on disk; anything else goes through the file, as in the reference
            resident = i_frame > 1 and last_key == (frame_width, frame_height, i_frame - 1) and state_sig == _file_sig(p(STATE_FILE))
            try:
                state_in = None if (resident or i_frame <= 1) else get_state_in_from_one_file(p(STATE_FILE), num_vectors, i_frame,
                                                                                               (frame_width, frame_height))
            except StaleStateError as exc:
                sys.stderr.write('resi_to_cu_depth_LDP: %s\n' % exc)
                if not accept_stale:
                    raise
                os.remove(p(STATE_FILE) + STATE_INDEX_SUFFIX)  # accepted: state.dat is taken as it is, as the reference would
                state_in = get_state_in_from_one_file(p(STATE_FILE), num_vectors, i_frame, (frame_width, frame_height))
            if state_in is not None:
                state_in = np.asarray(state_in, dtype=np.float32).reshape(num_vectors, 2, VECTOR_LENGTH)
            depth_out = ctx.ldp_step(luma, frame_width, frame_height, qp_seq, i_frame, state_in,
                                     probs_out=pinned_probs[:num_vectors * 21].reshape(num_vectors, 21))
            if pacer is not None:   # (only once the step has succeeded: a frame is never paced twice)
                if i_frame <= 1 or paced_geom != (frame_width, frame_height):
                    pacer.reset()   # a new sequence starts with a new allowance, as it starts with a zero LSTM state
                    paced_geom = (frame_width, frame_height)
                depth_out, res = pacer.frame(depth_out, frame_width, frame_height, out=depth_out)   # page-locked, in place
                paced = [paced[0] + 1, paced[1] + int(res['over']), paced[2] + int(res['cost']), paced[3] + int(res['full'])]
                if verbose:
                    print('frame %d: rung %d, %.6f of the full search%s' % (i_frame, int(res['rung']), int(res['cost']) / float(int(res['full']) or 1),
                                                                           ', over budget' if res['over'] else ''))
            save_cu_depth_and_state(depth_out, lambda: ctx.ldp_get_state(frame_width, frame_height), p(SAVE_FILE),
                                    p(STATE_FILE), p(END_FILE), num_vectors, tag=(i_frame, frame_width, frame_height))
            last_key, state_sig = (frame_width, frame_height, i_frame), _file_sig(p(STATE_FILE))
            n_frame_total += 1
            idle_since = time.time()
            if verbose:
                print('%d frames predicted.' % n_frame_total)
        return n_frame_total
    finally:
        if pacer is not None:
            sys.stderr.write('resi_to_cu_depth_LDP: search budget %g (%s): %.6f of the full search over %d frames, %d over budget\n'
                             % (budget[0], budget[1], paced[2] / float(paced[3] or 1), paced[0], paced[1]))
        ctx.close()


MAX_SESSIONS = 32   # ethcnn_ldp_sessions: sessions open at once
MAX_BUNDLES = 8     # ... and its bundle places


def check_sessions(workdirs, gates_per_dir=False):
    """What `--sessions` refuses at start-up, as ValueError, before a GPU is touched and with nothing written -> the gate thresholds
    all directories share.  The gates are the context's: every Thr_info.txt must give the first directory's gate tokens [1] and [3].
    gates_per_dir (`--gates-per-dir`): the files may differ, each must parse -> the list of every directory's pair, in their order."""
    budget = sorted(k for k in os.environ if k.startswith('ETHCNN_SEARCH_BUDGET'))
    if budget:
        raise ValueError('--sessions does not pace: %s is set, and the search budget is held per sequence (one daemon per encoder does that)'
                         % ', '.join(budget))
    if not workdirs:
        raise ValueError('--sessions needs at least one directory')
    if len(workdirs) > MAX_SESSIONS:
        raise ValueError('--sessions: %d directories, one server holds at most %d sessions' % (len(workdirs), MAX_SESSIONS))
    seen = {}
    for d in workdirs:
        real = os.path.realpath(d)
        if real in seen:
            raise ValueError('--sessions: %s is listed twice (as %s and %s)' % (real, seen[real], d))
        seen[real] = d
    gates, pairs = None, []
    for d in workdirs:
        path = os.path.join(d, THR_FILE)
        try:
            g = _e.parse_thresholds(path)
        except _e.EthCnnError:
            raise ValueError('--sessions: cannot read the thresholds of %s' % path)
        pairs.append(g)
        if gates_per_dir:
            continue
        if gates is None:
            gates = g
        elif g != gates:
            raise ValueError('--sessions: the gate thresholds of %s (%g %g) differ from those of %s (%g %g); one server has one pair of gates'
                             % (path, g[0], g[1], os.path.join(workdirs[0], THR_FILE), gates[0], gates[1]))
    return pairs if gates_per_dir else gates


def check_pace(workdirs, share, mode=None, weights=None, ladder=None):
    """What `--sessions ... --budget` refuses at start-up beyond check_sessions, as ValueError, before a GPU is touched and with nothing
    written: the four option values under search_budget's rules, and a directory whose Thr_info.txt is not the companion line in
    Low-Delay-P token order -> (share, mode, weights or None, ladder or None)"""
    names = _sb.OPTION_NAMES
    budget = _sb.from_values(share, mode, weights, names)
    if budget is None:
        raise ValueError("%s='' is not a share of the full search, 0..1" % names[0])
    rungs = _sb.ladder_from_path(ladder, 'ldp', auto=NO_AUTO_LADDER, name=names[3])
    for d in workdirs:
        _sb.check_companion_thr_file(os.path.join(d, THR_FILE), _sb.COMPANION_LINE_LDP, names[0])
    return budget + (rungs,)


def check_policies(workdirs, path, pace=None):
    """What `--sessions ... --budget-policies FILE` refuses at start-up beyond check_sessions (and check_pace, which gave `pace`, the
    default policy of the --budget options, or None), as ValueError, before a GPU is touched and with nothing written: a file that
    cannot be read or is malformed, a value search_budget refuses, `auto` as a ladder, a dir= line that names no directory of the server
    or one a second time, more than 32 policies, a directory that could be left without a policy, a rule of the library's own
    (ethcnn_pacer_policies_check), and a Thr_info.txt that is not the companion line -> search_budget.Policies"""
    name = _sb.POLICIES_OPTION
    policies = _sb.Policies(_sb.read_policies(path, 'ldp', auto=NO_AUTO_LADDER), workdirs, pace)
    try:
        _e.pacer_set_check_policies(_policy_dicts(policies.policies))
    except _e.EthCnnError as err:
        raise ValueError('%s: %s' % (name, err))
    for d in workdirs:
        _sb.check_companion_thr_file(os.path.join(d, THR_FILE), _sb.COMPANION_LINE_LDP, name)
    return policies


def _policy_dicts(policies):
    """search_budget's (share, mode, weights, ladder) tuples as ethcnn.PacerSet takes them"""
    return [{'budget': p[0], 'mode': p[1], 'weights': p[2], 'ladder': None if p[3] is None else _e.sim_thr(*p[3])} for p in policies]


class _BundlePlace(object):
    """bundle i of an LdpSessions object behind the two loaders restore_lstm calls"""

    def __init__(self, sessions, i):
        self.sessions, self.i = sessions, i

    def load_lstm_checkpoint(self, prefix):
        self.sessions.load_lstm_checkpoint(self.i, prefix)

    def load_lstm_synthetic(self, seed, head_gain):
        self.sessions.load_lstm_synthetic(self.i, seed, head_gain)


class _Dir(object):
    """one working directory of serve_many: its session, its page-locked buffers and what serve keeps per daemon"""

    def __init__(self, workdir):
        self.workdir = workdir
        self.session, self.geom = None, None
        self.last_key, self.state_sig = None, None
        self.pinned, self.pinned_probs = None, None
        self.paced_geom, self.paced = None, [0, 0, 0, 0]   # as serve's: frames, over budget, sum of cost, sum of full
        self.policy = None   # under --budget-policies: the (share, mode, weights, ladder) its slot is bound to
        self.gates = None    # under --gates-per-dir: the pair of its own Thr_info.txt, set on every session it opens

    def p(self, name):
        return os.path.join(self.workdir, name)


def _host_buffer_again(ctx, old, nbytes):
    """a page-locked buffer of nbytes in place of `old` (None: a first one)"""
    if old is not None:
        ctx.free_host_buffer(old)
    return ctx.host_buffer(nbytes)


def serve_many(workdirs, max_frames=None, idle_timeout=None, poll_s=2e-4, device=0, verbose=True, accept_stale=False, pace=None, policies=None,
               gates_per_dir=False):
    """One server for several HM working directories: one context, one LdpSessions object, the unchanged file handshake per directory.
    A poll round takes every directory with pred_start.sig and a complete command.dat, reads their resi.yuv, advances all of them
    in ONE step, writes cu_depth.dat and pred_end.sig per directory and then refreshes every served state.dat and its sidecar.  State
    continuity per directory is serve's rule.  max_frames and idle_timeout count over all directories.  Returns the frames predicted.
    pace: what check_pace returned, or None.  With it the gates are open and one PacerSet holds the search of every directory under that
    share: a directory's session id is its slot, and behind each step ONE call paces the round's frames in place in their page-locked
    buffers before the files are written.  A directory's slot is reset where serve resets its pacer.
    policies: what check_policies returned, or None.  With it the set holds every policy of the file (and `pace` as the default one), and
    where a directory's slot would be reset it is BOUND to the policy of that directory and of the QP of the frame that starts the
    allowance; the binding holds until the next start.
    gates_per_dir: every directory's session runs under the gate pair of that directory's own Thr_info.txt, as read at start-up; the
    context keeps the first directory's.  Without effect under pace or policies: the gates are then open for every directory."""
    gates = check_sessions(workdirs, gates_per_dir)
    dirs = [_Dir(d) for d in workdirs]
    if gates_per_dir and pace is None and policies is None:
        for d, g in zip(dirs, gates):
            d.gates = g
    ctx = _e.EthCnn(device=device)
    sessions = pacer = None
    try:
        ctx.load_thresholds(dirs[0].p(THR_FILE))   # (the gates check_sessions compared)
        if policies is not None:
            ctx.set_thresholds(0.0, 0.0)    # open gates, as below
            pacer = _e.PacerSet(ctx, MAX_SESSIONS, policies=_policy_dicts(policies.policies))
        elif pace is not None:
            ctx.set_thresholds(0.0, 0.0)    # open gates, whatever Thr_info.txt says: the baked files are what the encoders read
            pacer = _e.PacerSet(ctx, MAX_SESSIONS, pace[0], pace[1], ladder=None if pace[3] is None else _e.sim_thr(*pace[3]), weights=pace[2])
        restore_cnn(ctx, workdirs[0])
        sessions = _e.LdpSessions(ctx, MAX_BUNDLES)
        bundles = {}  # model name of a QP band -> bundle index
        if verbose:
            print('Python: predictor initialized on %s for %d directories.' % (ctx.device_name, len(dirs)))
        n_frame_total = 0
        idle_since = time.time()
        while max_frames is None or n_frame_total < max_frames:
            ready = []
            for d in dirs:
                if max_frames is not None and n_frame_total + len(ready) >= max_frames:
                    break
                if not os.path.isfile(d.p(START_FILE)):
                    continue
                cmd = get_command(d.p(COMMAND_FILE))
                if cmd[0] >= 0:
                    ready.append((d, cmd))
            if not ready:
                if idle_timeout is not None and time.time() - idle_since > idle_timeout:
                    break
                time.sleep(poll_s)
                continue
            frames = []
            for d, (i_frame, w, h, qp) in ready:
                os.remove(d.p(START_FILE))
                name = _e.lstm_model_name_for_qp(qp)
                if name not in bundles:
                    if len(bundles) == MAX_BUNDLES:
                        raise IOError('--sessions: more than %d QP bands in use' % MAX_BUNDLES)
                    loaded = restore_lstm(_BundlePlace(sessions, len(bundles)), qp, d.workdir)
                    bundles[name] = len(bundles)
                    if verbose:
                        print('LSTM model loaded for QP %d (%s).' % (qp, loaded))
                if d.geom != (w, h):  # a new sequence in this directory: a new session
                    if d.session is not None:
                        sessions.close(d.session)
                    d.session, d.geom, d.last_key, d.paced_geom = sessions.open(w, h), (w, h), None, None
                    if d.gates is not None:   # (a closed id forgets its pair: every open sets it again)
                        sessions.set_thresholds(d.session, d.gates[0], d.gates[1])
                num_vectors = _e.ctus_per_frame(w, h)
                if d.pinned is None or d.pinned.size < w * h:
                    d.pinned = _host_buffer_again(ctx, d.pinned, w * h)
                if d.pinned_probs is None or d.pinned_probs.size < num_vectors * 21:
                    d.pinned_probs = _host_buffer_again(ctx, d.pinned_probs, num_vectors * 21 * 4).view(np.float32)
                luma, _ = get_images_from_one_file(d.p(YUV_FILE), w, h, IMAGE_SIZE, into=d.pinned)
                resident = i_frame > 1 and d.last_key == (w, h, i_frame - 1) and d.state_sig == _file_sig(d.p(STATE_FILE))
                try:
                    state_in = None if (resident or i_frame <= 1) else get_state_in_from_one_file(d.p(STATE_FILE), num_vectors, i_frame, (w, h))
                except StaleStateError as exc:
                    sys.stderr.write('resi_to_cu_depth_LDP: %s\n' % exc)
                    if not accept_stale:
                        raise
                    os.remove(d.p(STATE_FILE) + STATE_INDEX_SUFFIX)
                    state_in = get_state_in_from_one_file(d.p(STATE_FILE), num_vectors, i_frame, (w, h))
                if state_in is not None:
                    state_in = np.asarray(state_in, dtype=np.float32).reshape(num_vectors, 2, VECTOR_LENGTH)
                frames.append({'session': d.session, 'luma': luma, 'qp': qp, 'i_frame': i_frame, 'bundle': bundles[name], 'state_in': state_in,
                               'probs_out': d.pinned_probs[:num_vectors * 21]})
            depths = sessions.step(frames)
            if pacer is not None:   # (only once the step has succeeded: a frame is never paced twice)
                for d, (i_frame, w, h, qp) in ready:
                    if i_frame <= 1 or d.paced_geom != (w, h):
                        if policies is None:
                            pacer.reset(d.session)   # a new sequence starts with a new allowance, as it starts with a zero LSTM state
                        else:   # ... and under the policy of this directory and of the QP it starts with, until the next start
                            d.policy = policies.policies[policies.of(d.workdir, qp)]
                            pacer.bind(d.session, policies.of(d.workdir, qp))
                        d.paced_geom = (w, h)
                depths, results = pacer.frames([{'slot': d.session, 'probs': depth, 'width': w, 'height': h, 'out': depth}   # page-locked, in place
                                                for depth, (d, (i_frame, w, h, qp)) in zip(depths, ready)])
                for res, (d, (i_frame, w, h, qp)) in zip(results, ready):
                    d.paced = [d.paced[0] + 1, d.paced[1] + int(res['over']), d.paced[2] + int(res['cost']), d.paced[3] + int(res['full'])]
                    if verbose:
                        print('%s: frame %d: rung %d, %.6f of the full search%s%s' % (d.workdir, i_frame, int(res['rung']),
                                                                                     int(res['cost']) / float(int(res['full']) or 1),
                                                                                     ', over budget' if res['over'] else '',
                                                                                     ' (budget %g, %s)' % d.policy[:2] if d.policy else ''))
            # what the encoders wait for first, for every directory; the state files afterwards, while they are encoding
            late = [save_cu_depth(depth, d.p(SAVE_FILE), d.p(STATE_FILE), d.p(END_FILE), _e.ctus_per_frame(w, h), (i_frame, w, h))
                    for depth, (d, (i_frame, w, h, qp)) in zip(depths, ready)]
            for finish, (d, (i_frame, w, h, qp)) in zip(late, ready):
                finish(sessions.get_state(d.session).reshape(-1, LSTM_DEPTH, 2, VECTOR_LENGTH))
                d.last_key, d.state_sig = (w, h, i_frame), _file_sig(d.p(STATE_FILE))
            n_frame_total += len(ready)
            idle_since = time.time()
            if verbose:
                print('%d frames predicted (%d in this step).' % (n_frame_total, len(ready)))
        return n_frame_total
    finally:
        for d in dirs:
            if d.paced[0]:
                sys.stderr.write('resi_to_cu_depth_LDP: %s: search budget %g (%s): %.6f of the full search over %d frames, %d over budget\n'
                                 % (d.workdir, (d.policy or pace)[0], (d.policy or pace)[1], d.paced[2] / float(d.paced[3] or 1), d.paced[0], d.paced[1]))
        if pacer is not None:
            pacer.close()
        if sessions is not None:
            sessions.close()
        ctx.close()


USAGE = ('usage: resi_to_cu_depth_LDP.py [--max-frames N] [--idle-timeout S] [--accept-stale]\n'
         '       resi_to_cu_depth_LDP.py --sessions DIR [DIR ...] [--max-frames N] [--idle-timeout S] [--accept-stale] [--quiet]\n'
         '                               [--budget SHARE [--budget-mode frame|carry] [--budget-weights "W64 W32 W16 W8"] [--budget-ladder FILE]]\n'
         '                               [--budget-policies FILE] [--gates-per-dir]\n')


def main(argv):
    """`python resi_to_cu_depth_LDP.py` in HM-LDP's bin/ (no arguments, like the reference);
    optional: --max-frames N, --idle-timeout SECONDS; --sessions DIR [DIR ...]: one server for several working directories, and behind
    it only --budget SHARE [--budget-mode M] [--budget-weights "W64 W32 W16 W8"] [--budget-ladder FILE]: the search budget of all of them,
    --budget-policies FILE: a policy per directory (the --budget options are then the default policy), --gates-per-dir: every directory
    under the gate thresholds of its own Thr_info.txt (no effect beside a budget: the gates are then open), and --quiet."""
    max_frames = idle = None
    accept_stale = quiet = gates_per_dir = False
    workdirs = None
    options = {}   # --budget, --budget-mode, --budget-weights, --budget-ladder -> their texts
    policy_file = None
    args = list(argv[1:])
    while args:
        a = args.pop(0)
        if a == '--max-frames' and args:
            max_frames = int(args.pop(0))
        elif a == '--idle-timeout' and args:
            idle = float(args.pop(0))
        elif a == '--accept-stale':
            accept_stale = True
        elif a == '--sessions' and workdirs is None:
            workdirs = []
            while args and not args[0].startswith('--'):
                workdirs.append(args.pop(0))
        elif a in _sb.OPTION_NAMES and a not in options and args:
            options[a] = args.pop(0)
        elif a == _sb.POLICIES_OPTION and policy_file is None and args:
            policy_file = args.pop(0)
        elif a == '--quiet':
            quiet = True
        elif a == '--gates-per-dir':
            gates_per_dir = True
        else:
            sys.stderr.write(USAGE)
            return 2
    if (options or quiet or gates_per_dir or policy_file is not None) and workdirs is None or (options and _sb.OPTION_NAMES[0] not in options):
        sys.stderr.write(USAGE)   # the budget options belong to --sessions, and the three others to --budget
        return 2
    if workdirs is not None:
        pace = policies = None
        try:
            check_sessions(workdirs, gates_per_dir)
            if options:
                pace = check_pace(workdirs, *[options.get(n) for n in _sb.OPTION_NAMES])
            if policy_file is not None:
                policies = check_policies(workdirs, policy_file, pace)
        except ValueError as err:
            sys.stderr.write('resi_to_cu_depth_LDP: %s\n' % err)
            return 1
        try:
            serve_many(workdirs, max_frames=max_frames, idle_timeout=idle, accept_stale=accept_stale, verbose=not quiet, pace=pace, policies=policies,
                       gates_per_dir=gates_per_dir)
        except StaleStateError:
            return 1
        return 0
    try:  # a bad ETHCNN_SEARCH_BUDGET* value, or a Thr_info.txt that is not the companion line: refused before a GPU is touched
        if _sb.from_env() is not None:
            _sb.ladder_from_env('ldp', auto=NO_AUTO_LADDER)
            _sb.check_companion_thr_file(THR_FILE, _sb.COMPANION_LINE_LDP)
    except ValueError as err:
        sys.stderr.write('resi_to_cu_depth_LDP: %s\n' % err)
        return 1
    try:
        serve('.', max_frames=max_frames, idle_timeout=idle, accept_stale=accept_stale)
    except StaleStateError:
        return 1  # (the message, with the recovery step, is already on stderr)
    return 0
