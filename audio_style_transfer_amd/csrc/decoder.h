// The decoder context shared by decoder.hip (the step form) and decoder_score.hip (the
// teacher-forced sequence form): one set of packed weights serves both.
#pragma once
#include <stddef.h>
#include <string>
#include <vector>

#include "../../include/astyle.h"

struct ast_dec {
    ast_dec_cfg c;
    int dev = 0, ntile = 0;
    char* ws = nullptr;
    size_t ws_bytes = 0;
    float *A_skip0, *wstart, *bstart, *bskip0;
    float *A_gate, *bdil, *bcond, *A_mix, *bres, *bskip;
    float *A1, *b1, *bc1, *A2, *b2, *tab_audio, *tab_xs;
    float *l, *s, *d, *ring, *xq;
    int* pos;
    std::vector<size_t> ring_off;   // floats, per layer
    size_t gate_sz = 0, mix_sz = 0; // floats per layer
};

namespace ast {
int set_error(int code, const std::string& msg);   // api.hip
int dec_check_cfg(const ast_dec_cfg* c);           // decoder.hip: 0, or AST_E_ARG with a message
}
