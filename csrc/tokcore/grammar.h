// response_format: the byte-level pushdown matcher of engine/grammar.py in C++ (same node table, same frames, same
// masks bit for bit) and the vocabulary's byte trie. No pybind11 here: tokcore.cpp binds it, csrc/tools/grammar_check.cpp
// links it into a stand-alone program.
//
// A state is a sorted set of stacks; a stack is a vector of frames, top last:
//   L (literal id, offset) / S (state, count, min, max) / N (state, digits, integer?) / W (k) read bytes;
//   V (node) / O (node, next member, first?) / F (first?) / A (node, items) are expanded until one of those is on top.
#pragma once
#include <cstdint>
#include <set>
#include <string>
#include <utility>
#include <vector>

namespace nlsgrammar {

constexpr int MAX_DEPTH = 64, MAX_INT_DIGITS = 16, MAX_FRAC_DIGITS = 16, MAX_EXP_DIGITS = 3, MAX_INDENT = 16;
constexpr int ANY = 0, ANY_ARRAY = 1, ANY_OBJECT = 2;      // nodes every table begins with

enum NodeKind : int32_t { N_LIT = 0, N_ALT, N_STR, N_NUM, N_OBJ, N_FOBJ, N_ARR, N_ANY };
enum FrameKind : int32_t { F_L = 0, F_S, F_N, F_W, F_V, F_O, F_F, F_A };

struct Frame {
  int32_t k, a, b, c, d;
  bool operator<(const Frame& o) const {
    if (k != o.k) return k < o.k;
    if (a != o.a) return a < o.a;
    if (b != o.b) return b < o.b;
    if (c != o.c) return c < o.c;
    return d < o.d;
  }
  bool operator==(const Frame& o) const { return k == o.k && a == o.a && b == o.b && c == o.c && d == o.d; }
};
using Stack = std::vector<Frame>;
using State = std::vector<Stack>;      // sorted, distinct

// nodes[i]: [N_LIT, literal] / [N_ALT, node...] / [N_STR, min, max] / [N_NUM, integer?] /
//           [N_OBJ, (key literal, node, required?)...] / [N_FOBJ] / [N_ARR, item, min, max] / [N_ANY]; max -1: unbounded.
// punct: the literal ids of  " : , [ ] { } true false null
struct Grammar {
  std::vector<std::vector<int32_t>> nodes;
  std::vector<std::string> lits;
  std::vector<int32_t> mind;
  int32_t root = 0;
  int32_t punct[10] = {0};

  bool valid() const;                    // every index the matcher will follow is in range
  State start() const;
  State step(const State& s, uint8_t b) const;

 private:
  void value(int32_t node, int depth, std::vector<Stack>& runs) const;
  void expand(Stack& st, std::set<Stack>& out) const;
  bool consume(Stack& st, uint8_t b) const;
};

struct Vocab {
  struct TNode {
    std::vector<std::pair<uint8_t, int32_t>> kids;
    std::vector<int32_t> toks;
  };
  std::vector<std::string> token_bytes;      // "": never allowed by its bytes (the eog ids among them)
  std::vector<int32_t> eog;
  int32_t n_vocab = 0;
  std::vector<TNode> trie;

  Vocab(std::vector<std::string> tb, std::vector<int32_t> eog_ids, int32_t n);
  int32_t n_words() const { return (n_vocab + 31) / 32; }
  bool is_eog(int32_t t) const;
};

class Matcher {
 public:
  Matcher(const Grammar* g, const Vocab* v) : g_(g), v_(v), state_(g->start()) {}
  bool advance(int32_t token);
  bool is_complete() const;
  void fill_mask(uint32_t* words) const;     // n_words() words, overwritten
  std::string state_key() const;

 private:
  const Grammar* g_;
  const Vocab* v_;
  State state_;
  bool ended_ = false;
};

uint64_t checksum(const uint32_t* words, int n);      // FNV-1a over the words' little-endian bytes

}  // namespace nlsgrammar
