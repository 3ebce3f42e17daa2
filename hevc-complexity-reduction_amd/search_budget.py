"""The environment of the search budget (include/ethcnn.h "search budget"), shared by the launchers that take one: the All-Intra
launcher (video_to_cu_depth.py) and the Low-Delay-P daemon (resi_to_cu_depth_LDP.py).  ETHCNN_SEARCH_BUDGET=<share, 0..1>,
ETHCNN_SEARCH_BUDGET_MODE=frame|carry (default frame), ETHCNN_SEARCH_BUDGET_WEIGHTS="64 16 4 1", ETHCNN_SEARCH_BUDGET_LADDER=<ladder file>
(default: the default ladder; read only when a budget is set).  ETHCNN_SEARCH_BUDGET_LADDER=auto asks a launcher that sees the whole
sequence before the encoder starts to build the ladder itself, without labels, from its own predictions (include/ethcnn.h
"partition-search simulation: expected wrong decisions"); ETHCNN_SEARCH_BUDGET_RELIABILITY=<table file> is then optional.  Nothing here
touches a GPU."""
import os

COMPANION_LINE_AI = '0.75 0.25 0.75 0.25 0.75 0.25'    # ethcnn_budget_companion_thr in All-Intra token order: up down ...
COMPANION_LINE_LDP = '0.25 0.75 0.25 0.75 0.25 0.75'   # ... and in Low-Delay-P token order: down up ...
MAX_RUNGS = 4096                                       # ETHCNN_BUDGET_MAX_RUNGS
AUTO = 'auto'                                          # ETHCNN_SEARCH_BUDGET_LADDER=auto: a ladder built from the sequence itself
AUTO_GRID = 8                                          # ... on this grid, up to MAX_RUNGS rungs, without a cap


ENV_NAMES = ('ETHCNN_SEARCH_BUDGET', 'ETHCNN_SEARCH_BUDGET_MODE', 'ETHCNN_SEARCH_BUDGET_WEIGHTS', 'ETHCNN_SEARCH_BUDGET_LADDER')
OPTION_NAMES = ('--budget', '--budget-mode', '--budget-weights', '--budget-ladder')   # the same four as command-line options


def from_values(share_text, mode_text, weights_text, names=ENV_NAMES):
    """None when the share is unset or empty, else (share, mode, weights or None); ValueError names a bad value after `names`, the
    variables or options the three texts came from"""
    text = share_text
    if text is None or text == '':
        return None
    try:
        share = float(text)
    except ValueError:
        share = -1.0
    if not 0.0 <= share <= 1.0:   # (a NaN fails both comparisons)
        raise ValueError("%s='%s' is not a share of the full search, 0..1" % (names[0], text))
    mode = mode_text or 'frame'
    if mode not in ('frame', 'carry'):
        raise ValueError("%s='%s' (allowed: frame, carry)" % (names[1], mode))
    weights = None
    text = weights_text
    if text:
        try:
            weights = [int(t) for t in text.split()]
        except ValueError:
            weights = []
        if len(weights) != 4 or min(weights) < 0 or max(weights) >= 1 << 32:
            raise ValueError("%s='%s' is not four integers W64 W32 W16 W8 in 0..2^32-1" % (names[2], text))
    return share, mode, weights


def from_env():
    """None when ETHCNN_SEARCH_BUDGET is unset or empty, else (share, mode, weights or None); ValueError names a bad value"""
    return from_values(*[os.environ.get(n) for n in ENV_NAMES[:3]])


def check_companion_thr_file(path, line, name=ENV_NAMES[0]):
    """A baked cu_depth.dat means what it says only under the companion thresholds, and HM reads them from this file: ValueError unless
    it holds exactly the six values of `line` (the companion line in the token order of the encoder that reads it)"""
    try:
        tokens = [float(t) for t in open(path).read().split()]
    except (OSError, ValueError):
        tokens = None
    if tokens != [float(t) for t in line.split()]:
        raise ValueError("%s is set, so the encoder must read the companion thresholds: put the line\n    %s\ninto %s "
                         "(found: %s)" % (name, line, path, 'no readable file' if tokens is None else ' '.join('%g' % t for t in tokens)))


def read_ladder(path, order):
    """a ladder file (ethcnn_ladder_write, tools/build_ladder.py --out): one rung per line, six values in the token order `order`
    ('ai': up down ..., 'ldp': down up ...), the most thorough first -> (up_k [K][3], down_k [K][3]) on the grid; ValueError names the
    line, OSError a file that cannot be read"""
    up, down = [], []
    for no, line in enumerate(open(path).read().splitlines(), 1):
        tok = line.split()
        if not tok:
            continue
        try:
            k = [int(round(float(t) * 1024)) for t in tok]
        except (ValueError, OverflowError):
            k = []
        if len(k) != 6:
            raise ValueError("%s, line %d: a rung is six values" % (path, no))
        a, b = k[0::2], k[1::2]
        u, d = (a, b) if order == "ai" else (b, a)
        if min(u) < 0 or max(u) > 1024 or min(d) < -1 or max(d) > 1024:
            raise ValueError("%s, line %d: thresholds outside [0, 1] (down: [-1/1024, 1])" % (path, no))
        up.append(u)
        down.append(d)
    if not 1 <= len(up) <= MAX_RUNGS:
        raise ValueError("%s: a ladder has 1..%d rungs, got %d" % (path, MAX_RUNGS, len(up)))
    return up, down


def ladder_from_path(path, order, auto=None, name=ENV_NAMES[3]):
    """None when `path` is unset or empty (the default ladder), else read_ladder of that file in the token order of the launcher that
    asks; ValueError names a file that is missing or malformed or holds more than 4096 rungs, after `name`, the variable or option the
    path came from.  The value "auto" gives AUTO to a launcher that can build a ladder from the sequence it is about to predict
    (auto=True); every other launcher passes the reason why it cannot, and the ValueError carries it"""
    if not path:
        return None
    if path == AUTO and auto is not None:
        if auto is True:
            return AUTO
        raise ValueError("%s='auto' cannot be read: %s" % (name, auto))
    try:
        return read_ladder(path, order)
    except OSError as err:
        raise ValueError("%s='%s' cannot be read: %s" % (name, path, err.strerror or err))
    except ValueError as err:
        raise ValueError("%s: %s" % (name, err))


def ladder_from_env(order, auto=None):
    """ladder_from_path of ETHCNN_SEARCH_BUDGET_LADDER"""
    return ladder_from_path(os.environ.get(ENV_NAMES[3]), order, auto)


MAX_POLICIES = 32                                      # ETHCNN_PACER_SET_MAX_POLICIES
POLICIES_OPTION = '--budget-policies'


def read_policies(path, order, auto=None, name=POLICIES_OPTION):
    """a policy file of `--sessions ... --budget-policies`: one policy per line, `#` starts a comment, whitespace-separated fields
    SELECTOR SHARE [MODE [LADDER|- [W64 W32 W16 W8]]].  SELECTOR is dir=PATH, qp=LO..HI (inclusive) or *; SHARE, MODE and the weights are
    under from_values' rules, LADDER is a ladder file in the token order `order` (`-`: the default ladder; `auto` is refused with the
    reason `auto`) -> one (selector, (share, mode, weights or None, ladder or None)) per line, selector one of ('dir', realpath),
    ('qp', lo, hi), ('*',); ValueError names the file and the line"""
    try:
        lines = open(path).read().splitlines()
    except (OSError, UnicodeDecodeError) as err:
        raise ValueError("%s='%s' cannot be read: %s" % (name, path, getattr(err, 'strerror', None) or err))
    out = []
    for no, line in enumerate(lines, 1):
        tok = line.split('#', 1)[0].split()
        if not tok:
            continue
        at = '%s, line %d' % (path, no)
        if len(tok) not in (2, 3, 4, 8):
            raise ValueError("%s: %s: a policy is SELECTOR SHARE [MODE [LADDER|- [W64 W32 W16 W8]]], got %d fields" % (name, at, len(tok)))
        sel = tok[0]
        if sel == '*':
            selector = ('*',)
        elif sel.startswith('dir=') and len(sel) > 4:
            selector = ('dir', os.path.realpath(sel[4:]))
        elif sel.startswith('qp='):
            try:
                lo, hi = [int(t) for t in sel[3:].split('..')]
            except ValueError:
                raise ValueError("%s: %s: '%s' is not qp=LO..HI" % (name, at, sel))
            if lo > hi:
                raise ValueError("%s: %s: '%s' is an empty range (LO > HI)" % (name, at, sel))
            selector = ('qp', lo, hi)
        else:
            raise ValueError("%s: %s: the selector '%s' is none of dir=PATH, qp=LO..HI and *" % (name, at, sel))
        try:
            budget = from_values(tok[1], tok[2] if len(tok) > 2 else None, ' '.join(tok[4:]) if len(tok) > 4 else None,
                                 (at + ': SHARE', at + ': MODE', at + ': W64 W32 W16 W8'))
            ladder = ladder_from_path(tok[3] if len(tok) > 3 and tok[3] != '-' else None, order, auto, at + ': LADDER')
        except ValueError as err:
            raise ValueError('%s: %s' % (name, err))
        out.append((selector, budget + (ladder,)))
    return out


class Policies(object):
    """the policies of one server and the rule that gives a directory its own.  policies: (share, mode, weights or None, ladder or
    None) each, the lines of the file in file order and then the default of the --budget options, if there is one; at most
    MAX_POLICIES.  of(directory, qp) is the index of the first match in this order: the first dir= line whose realpath is the
    directory's, else the first qp= line that holds qp, else the first * line, else the --budget default."""

    def __init__(self, lines, workdirs, default=None, name=POLICIES_OPTION):
        """lines: what read_policies returned; ValueError for a dir= line that names none of `workdirs` or a directory a second time, for
        more than MAX_POLICIES policies, and for a directory that may be left without a policy"""
        self.policies = [p for _, p in lines] + ([default] if default is not None else [])
        if not self.policies:
            raise ValueError('%s: the file holds no policy and there is no --budget' % name)
        if len(self.policies) > MAX_POLICIES:
            raise ValueError('%s: %d policies%s, one server holds at most %d' % (name, len(self.policies), ', the --budget default among them' if default is not None else '',
                                                                                MAX_POLICIES))
        real = [os.path.realpath(d) for d in workdirs]
        self.by_dir, self.by_qp, self.fallback = {}, [], None
        for i, (sel, _) in enumerate(lines):
            if sel[0] == 'dir':
                if sel[1] not in real:
                    raise ValueError('%s: dir=%s names none of the --sessions directories' % (name, sel[1]))
                if sel[1] in self.by_dir:
                    raise ValueError('%s: two dir= lines for %s' % (name, sel[1]))
                self.by_dir[sel[1]] = i
            elif sel[0] == 'qp':
                self.by_qp.append((sel[1], sel[2], i))
            elif self.fallback is None:
                self.fallback = i
        if self.fallback is None and default is not None:
            self.fallback = len(self.policies) - 1
        if self.fallback is None:
            bare = [d for d, r in zip(workdirs, real) if r not in self.by_dir]
            if bare:
                raise ValueError('%s: %s has no dir= line and there is no default (a * line or --budget)' % (name, bare[0]))

    def of(self, directory, qp):
        real = os.path.realpath(directory)
        if real in self.by_dir:
            return self.by_dir[real]
        for lo, hi, i in self.by_qp:
            if lo <= qp <= hi:
                return i
        return self.fallback   # (never None for a directory of the server: __init__ refused that)


def reliability_from_env(read):
    """None when ETHCNN_SEARCH_BUDGET_RELIABILITY is unset or empty (the identity table), else read(path) -- the binding's risk_read,
    host only; ValueError names a file that cannot be read or is no reliability table"""
    path = os.environ.get('ETHCNN_SEARCH_BUDGET_RELIABILITY')
    if not path:
        return None
    try:
        return read(path)
    except (OSError, RuntimeError) as err:   # (libethcnn errors are RuntimeErrors)
        raise ValueError("ETHCNN_SEARCH_BUDGET_RELIABILITY='%s' cannot be read: %s" % (path, err))
