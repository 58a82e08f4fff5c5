// Stand-alone replay of the response_format matcher (csrc/tokcore/grammar.cpp), for sanitizer builds: no Python.
//
//   grammar_check <file>
//
// The file (written by tests/test_response_format.py) holds one vocabulary and any number of grammars with token paths:
//   V <n_vocab> <n_tokens> <n_eog>        then a line of eog ids, then one line per token: its bytes in hex, or "-"
//   G <n_nodes> <n_lits> <root> <n_paths> then 10 punctuation literal ids, the nodes' minimum depths, one line of ints
//                                         per node, one hex line per literal, and per path: <n> and its token ids
// For every path it prints the checksums of the masks in front of each token and behind the last one, on one line;
// a rejected token or a malformed file ends it with status 1.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "grammar.h"

namespace G = nlsgrammar;

static bool unhex(const std::string& s, std::string& out) {
  out.clear();
  if (s == "-") return true;
  if (s.size() % 2) return false;
  for (size_t i = 0; i < s.size(); i += 2) {
    int v = 0;
    for (int k = 0; k < 2; ++k) {
      const char c = s[i + k];
      v = v * 16 + (c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1000);
    }
    if (v < 0) return false;
    out.push_back((char)v);
  }
  return true;
}

static bool ints(std::istream& in, size_t n, std::vector<int32_t>& out) {
  out.assign(n, 0);
  for (auto& v : out)
    if (!(in >> v)) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: grammar_check <file>\n");
    return 2;
  }
  std::ifstream in(argv[1]);
  std::string tag, word;
  long nv = 0, nt = 0, ne = 0;
  if (!(in >> tag >> nv >> nt >> ne) || tag != "V" || nv < 0 || nt < 0 || ne < 0 || nt > (1 << 24)) return 1;
  std::vector<int32_t> eog;
  if (!ints(in, (size_t)ne, eog)) return 1;
  std::vector<std::string> toks((size_t)nt);
  for (auto& t : toks)
    if (!(in >> word) || !unhex(word, t)) return 1;
  const G::Vocab vocab(std::move(toks), eog, (int32_t)nv);
  std::vector<uint32_t> mask((size_t)vocab.n_words());
  long nn, nl, root, np;
  while (in >> tag >> nn >> nl >> root >> np) {
    if (tag != "G" || nn < 0 || nl < 0 || np < 0 || nn > (1 << 20) || nl > (1 << 20)) return 1;
    G::Grammar g;
    std::vector<int32_t> punct;
    if (!ints(in, 10, punct) || !ints(in, (size_t)nn, g.mind)) return 1;
    for (int i = 0; i < 10; ++i) g.punct[i] = punct[i];
    g.root = (int32_t)root;
    std::string line;
    std::getline(in, line);
    for (long i = 0; i < nn; ++i) {
      if (!std::getline(in, line)) return 1;
      std::istringstream ls(line);
      std::vector<int32_t> row;
      for (int32_t v; ls >> v;) row.push_back(v);
      g.nodes.push_back(row);
    }
    g.lits.resize((size_t)nl);
    for (auto& l : g.lits)
      if (!(in >> word) || !unhex(word, l)) return 1;
    if (!g.valid()) {
      std::fprintf(stderr, "grammar_check: malformed node table\n");
      return 1;
    }
    for (long p = 0; p < np; ++p) {
      long n;
      std::vector<int32_t> path;
      if (!(in >> n) || n < 0 || !ints(in, (size_t)n, path)) return 1;
      G::Matcher m(&g, &vocab);
      for (long i = 0; i <= n; ++i) {
        m.fill_mask(mask.data());
        std::printf("%s%016llx", i ? " " : "", (unsigned long long)G::checksum(mask.data(), (int)mask.size()));
        if (i < n && !m.advance(path[(size_t)i])) {
          std::fprintf(stderr, "\ngrammar_check: token %d rejected at step %ld of path %ld\n", path[(size_t)i], i, p);
          return 1;
        }
      }
      std::printf(" %s %zu\n", m.is_complete() ? "complete" : "open", m.state_key().size());
    }
  }
  return 0;
}
