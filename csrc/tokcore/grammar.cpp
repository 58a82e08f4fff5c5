// See grammar.h. The twin of nats_llm_studio_amd/engine/grammar.py (Grammar._value / _expand / _consume / step,
// CompiledGrammar._fill): change both together; tests/test_response_format.py compares their masks bit for bit.
#include "grammar.h"

#include <algorithm>
#include <cstring>

namespace nlsgrammar {

namespace {
enum { P_Q = 0, P_COLON, P_COMMA, P_LB, P_RB, P_LC, P_RC, P_TRUE, P_FALSE, P_NULL };

inline Frame L(int32_t lit) { return Frame{F_L, lit, 0, 0, 0}; }
inline Frame W() { return Frame{F_W, -1, 0, 0, 0}; }
inline Frame V(int32_t node) { return Frame{F_V, node, 0, 0, 0}; }

inline int depth_of(const Stack& st, size_t upto) {
  int d = 0;
  for (size_t i = 0; i < upto; ++i) d += st[i].k == F_O || st[i].k == F_F || st[i].k == F_A;
  return d;
}
}  // namespace

bool Grammar::valid() const {
  const int32_t nn = (int32_t)nodes.size(), nl = (int32_t)lits.size();
  if (nn < 3 || (int32_t)mind.size() != nn || root < 0 || root >= nn) return false;
  if (nodes[ANY].empty() || nodes[ANY][0] != N_ANY || nodes[ANY_ARRAY].empty() || nodes[ANY_ARRAY][0] != N_ARR ||
      nodes[ANY_OBJECT].empty() || nodes[ANY_OBJECT][0] != N_FOBJ)
    return false;
  for (int i = 0; i < 10; ++i)
    if (punct[i] < 0 || punct[i] >= nl) return false;
  for (const auto& s : lits)
    if (s.empty()) return false;
  for (const auto& n : nodes) {
    if (n.empty()) return false;
    switch (n[0]) {
      case N_LIT:
        if (n.size() != 2 || n[1] < 0 || n[1] >= nl) return false;
        break;
      case N_ALT:
        for (size_t i = 1; i < n.size(); ++i)
          if (n[i] < 0 || n[i] >= nn) return false;
        break;
      case N_STR:
        if (n.size() != 3 || n[1] < 0) return false;
        break;
      case N_NUM:
        if (n.size() != 2) return false;
        break;
      case N_OBJ:
        if ((n.size() - 1) % 3 != 0) return false;
        for (size_t i = 1; i < n.size(); i += 3)
          if (n[i] < 0 || n[i] >= nl || n[i + 1] < 0 || n[i + 1] >= nn) return false;
        break;
      case N_FOBJ:
      case N_ANY:
        break;
      case N_ARR:
        if (n.size() != 4 || n[1] < 0 || n[1] >= nn || n[2] < 0) return false;
        break;
      default:
        return false;
    }
  }
  return true;
}

void Grammar::value(int32_t node, int depth, std::vector<Stack>& runs) const {
  if (depth + mind[node] > MAX_DEPTH) return;
  const auto& n = nodes[node];
  switch (n[0]) {
    case N_LIT:
      runs.push_back({L(n[1])});
      break;
    case N_ALT:
      for (size_t i = 1; i < n.size(); ++i) value(n[i], depth, runs);
      break;
    case N_STR:
      runs.push_back({Frame{F_S, 0, 0, n[1], n[2]}, L(punct[P_Q])});
      break;
    case N_NUM:
      runs.push_back({Frame{F_N, 0, 0, n[1], 0}});
      break;
    case N_OBJ:
      runs.push_back({Frame{F_O, node, 0, 1, 0}, W(), L(punct[P_LC])});
      break;
    case N_FOBJ:
      runs.push_back({Frame{F_F, 1, 0, 0, 0}, W(), L(punct[P_LC])});
      break;
    case N_ARR:
      runs.push_back({Frame{F_A, node, 0, 0, 0}, W(), L(punct[P_LB])});
      break;
    default:      // any
      runs.push_back({Frame{F_S, 0, 0, 0, -1}, L(punct[P_Q])});
      runs.push_back({Frame{F_N, 0, 0, 0, 0}});
      runs.push_back({L(punct[P_TRUE])});
      runs.push_back({L(punct[P_FALSE])});
      runs.push_back({L(punct[P_NULL])});
      value(ANY_ARRAY, depth, runs);
      value(ANY_OBJECT, depth, runs);
  }
}

// st is taken apart and put together again: on return it holds what it held
void Grammar::expand(Stack& st, std::set<Stack>& out) const {
  if (st.empty()) {
    out.insert(st);
    return;
  }
  const Frame f = st.back();
  if (f.k == F_L || f.k == F_S) {
    out.insert(st);
    return;
  }
  if (f.k == F_N || f.k == F_W) {
    out.insert(st);
    if (f.k == F_W || f.a == 2 || f.a == 3 || f.a == 5 || f.a == 8) {
      st.pop_back();
      expand(st, out);
      st.push_back(f);
    }
    return;
  }
  const size_t base = st.size() - 1;
  auto with = [&](std::initializer_list<Frame> run, bool sep) {
    st.resize(base);
    st.insert(st.end(), run.begin(), run.end());
    if (sep) {
      st.push_back(W());
      st.push_back(L(punct[P_COMMA]));
    }
    expand(st, out);
  };
  if (f.k == F_V) {
    std::vector<Stack> runs;
    value(f.a, depth_of(st, base), runs);
    for (const auto& run : runs) {
      st.resize(base);
      st.insert(st.end(), run.begin(), run.end());
      expand(st, out);
    }
  } else {
    const int depth = depth_of(st, base) + 1;      // this container included
    const Frame close = L(f.k == F_A ? punct[P_RB] : punct[P_RC]);
    if (f.k == F_O) {
      const auto& n = nodes[f.a];
      const int32_t members = (int32_t)(n.size() - 1) / 3;
      bool open = true;
      for (int32_t j = f.b; j < members; ++j) {
        const int32_t key = n[1 + 3 * j], node = n[2 + 3 * j], req = n[3 + 3 * j];
        if (depth + mind[node] <= MAX_DEPTH)
          with({Frame{F_O, f.a, j + 1, 0, 0}, V(node), W(), L(punct[P_COLON]), L(key)}, !f.c);
        if (req) {
          open = false;
          break;
        }
      }
      if (open) with({close, W()}, false);
    } else if (f.k == F_F) {
      with({close, W()}, false);
      with({Frame{F_F, 0, 0, 0, 0}, V(ANY), W(), L(punct[P_COLON]), Frame{F_S, 0, 0, 0, -1}, L(punct[P_Q])}, !f.a);
    } else {
      const auto& n = nodes[f.a];
      const int32_t item = n[1], mn = n[2], mx = n[3], cnt = f.b;
      if (cnt >= mn) with({close, W()}, false);
      if ((mx < 0 || cnt < mx) && depth + mind[item] <= MAX_DEPTH) {
        const int32_t nn = mx >= 0 ? cnt + 1 : std::min(cnt + 1, std::max(mn, 1));      // unbounded: saturates
        with({Frame{F_A, f.a, nn, 0, 0}, V(item)}, cnt != 0);
      }
    }
  }
  st.resize(base);
  st.push_back(f);
}

// the stack behind byte b (its top frame reads bytes); false: rejected (st is then unspecified)
bool Grammar::consume(Stack& st, uint8_t b) const {
  Frame& f = st.back();
  switch (f.k) {
    case F_L: {
      const std::string& lit = lits[f.a];
      if ((uint8_t)lit[f.b] != b) return false;
      if (f.b + 1 == (int32_t)lit.size())
        st.pop_back();
      else
        ++f.b;
      return true;
    }
    case F_W:
      if (b == 0x20) {
        if (f.a < 0) {
          st.pop_back();
          return true;
        }
        if (f.a >= MAX_INDENT) return false;
        ++f.a;
        return true;
      }
      if (b == 0x0A && f.a < 0) {
        f.a = 0;
        return true;
      }
      return false;
    case F_N: {
      const int32_t s = f.a, cnt = f.b;
      const bool integer = f.c != 0, digit = b >= 0x30 && b <= 0x39, e = b == 0x65 || b == 0x45;
      int32_t ns = -1, nc = 0;
      if (s == 0 && b == 0x2D) {
        ns = 1;
      } else if (s == 0 || s == 1) {
        if (b == 0x30) ns = 2, nc = 1;
        else if (digit) ns = 3, nc = 1;
      } else if ((s == 2 || s == 3 || s == 5) && !integer && e) {
        ns = 6;
      } else if ((s == 2 || s == 3) && !integer && b == 0x2E) {
        ns = 4;
      } else if (s == 3 && digit) {
        if (cnt < MAX_INT_DIGITS) ns = 3, nc = cnt + 1;
      } else if ((s == 4 || s == 5) && digit) {
        if (s == 4 || cnt < MAX_FRAC_DIGITS) ns = 5, nc = cnt + 1;
      } else if (s == 6 && (b == 0x2B || b == 0x2D)) {
        ns = 7;
      } else if ((s == 6 || s == 7 || s == 8) && digit) {
        if (s != 8 || cnt < MAX_EXP_DIGITS) ns = 8, nc = cnt + 1;
      }
      if (ns < 0) return false;
      f.a = ns;
      f.b = nc;
      return true;
    }
    default: {      // F_S
      const int32_t s = f.a, mn = f.c, mx = f.d;
      int32_t ns;
      if (s == 0) {
        if (b == 0x22) {
          if (f.b < mn) return false;
          st.pop_back();
          return true;
        }
        if (b < 0x20 || (mx >= 0 && f.b >= mx)) return false;
        if (b == 0x5C) ns = 1;
        else if (b < 0x80) ns = 0;
        else if (b >= 0xC2 && b <= 0xDF) ns = 21;
        else if (b == 0xE0) ns = 30;
        else if (b == 0xED) ns = 31;
        else if (b >= 0xE1 && b <= 0xEF) ns = 22;
        else if (b == 0xF0) ns = 32;
        else if (b >= 0xF1 && b <= 0xF3) ns = 23;
        else if (b == 0xF4) ns = 33;
        else return false;
        f.b = mx < 0 ? std::min(f.b + 1, mn) : f.b + 1;      // unbounded: the count saturates at min
      } else if (s == 1) {
        if (b == 0x75) ns = 14;
        else if (std::strchr("\"\\/bfnrt", (char)b) != nullptr && b != 0) ns = 0;
        else return false;
      } else if (s >= 11 && s <= 14) {
        if (!((b >= 0x30 && b <= 0x39) || (b >= 0x41 && b <= 0x46) || (b >= 0x61 && b <= 0x66))) return false;
        ns = s > 11 ? s - 1 : 0;
      } else if (s >= 21 && s <= 23) {
        if (b < 0x80 || b > 0xBF) return false;
        ns = s > 21 ? s - 1 : 0;
      } else {
        const uint8_t lo = s == 30 ? 0xA0 : s == 32 ? 0x90 : 0x80, hi = s == 31 ? 0x9F : s == 33 ? 0x8F : 0xBF;
        if (b < lo || b > hi) return false;
        ns = s <= 31 ? 21 : 22;
      }
      f.a = ns;
      return true;
    }
  }
}

State Grammar::start() const {
  std::set<Stack> out;
  Stack st{V(root)};
  expand(st, out);
  return State(out.begin(), out.end());
}

State Grammar::step(const State& s, uint8_t b) const {
  std::set<Stack> out;
  for (const Stack& stack : s) {
    if (stack.empty()) continue;
    Stack st = stack;
    if (consume(st, b)) expand(st, out);
  }
  return State(out.begin(), out.end());
}

Vocab::Vocab(std::vector<std::string> tb, std::vector<int32_t> eog_ids, int32_t n)
    : token_bytes(std::move(tb)), n_vocab(std::max<int32_t>(n, 0)) {
  n_vocab = std::max<int32_t>(n_vocab, (int32_t)token_bytes.size());
  for (int32_t e : eog_ids)
    if (e >= 0 && e < n_vocab) eog.push_back(e);
  std::sort(eog.begin(), eog.end());
  eog.erase(std::unique(eog.begin(), eog.end()), eog.end());
  for (int32_t e : eog)      // an end-of-generation id ends the request, whatever its type: never by its bytes
    if (e < (int32_t)token_bytes.size()) token_bytes[e].clear();
  trie.emplace_back();
  for (size_t t = 0; t < token_bytes.size(); ++t) {
    const std::string& bs = token_bytes[t];
    if (bs.empty()) continue;
    int32_t node = 0;
    for (unsigned char b : bs) {
      int32_t next = -1;
      for (const auto& kid : trie[node].kids)
        if (kid.first == b) {
          next = kid.second;
          break;
        }
      if (next < 0) {
        next = (int32_t)trie.size();
        trie[node].kids.emplace_back(b, next);
        trie.emplace_back();
      }
      node = next;
    }
    trie[node].toks.push_back((int32_t)t);
  }
}

bool Vocab::is_eog(int32_t t) const { return std::binary_search(eog.begin(), eog.end(), t); }

bool Matcher::advance(int32_t t) {
  if (ended_) return false;
  if (v_->is_eog(t)) {
    if (!is_complete()) return false;
    ended_ = true;
    return true;
  }
  if (t < 0 || t >= (int32_t)v_->token_bytes.size() || v_->token_bytes[t].empty()) return false;
  State s = state_;
  for (unsigned char b : v_->token_bytes[t]) {
    s = g_->step(s, b);
    if (s.empty()) return false;
  }
  state_ = std::move(s);
  return true;
}

bool Matcher::is_complete() const { return ended_ || (!state_.empty() && state_.front().empty()); }

void Matcher::fill_mask(uint32_t* words) const {
  const int nw = v_->n_words();
  std::fill(words, words + nw, 0u);
  auto allow = [&](int32_t t) { words[t >> 5] |= 1u << (t & 31); };
  if (is_complete())
    for (int32_t e : v_->eog) allow(e);
  if (ended_) return;
  // the trie walk: a branch is cut at its first rejected byte
  std::vector<std::pair<int32_t, State>> work;
  work.emplace_back(0, state_);
  while (!work.empty()) {
    const int32_t node = work.back().first;
    const State st = std::move(work.back().second);
    work.pop_back();
    for (const auto& kid : v_->trie[node].kids) {
      State ns = g_->step(st, kid.first);
      if (ns.empty()) continue;
      const Vocab::TNode& c = v_->trie[kid.second];
      for (int32_t t : c.toks) allow(t);
      if (!c.kids.empty()) work.emplace_back(kid.second, std::move(ns));
    }
  }
}

std::string Matcher::state_key() const {
  std::string key(ended_ ? "E" : "S");
  for (const Stack& st : state_) {
    const uint32_t n = (uint32_t)st.size();
    key.append((const char*)&n, sizeof n);
    if (n) key.append((const char*)st.data(), n * sizeof(Frame));
  }
  return key;
}

uint64_t checksum(const uint32_t* words, int n) {
  uint64_t h = 1469598103934665603ull;
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 4; ++k) {
      h ^= (words[i] >> (8 * k)) & 0xFFu;
      h *= 1099511628211ull;
    }
  return h;
}

}  // namespace nlsgrammar
