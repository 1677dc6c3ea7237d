# The client of the libjpeg DECOMPRESS API (TEST INFRASTRUCTURE, tests/test_simt_djpeg.py / tests/test_gpu_djpeg.py), built like the
# clients of ./Makefile: against the reference's headers, linked to the reference's library; the binary travels to the GPU box with the tree.
#   make -C tests/native -f djpeg_client.mk
REF ?= /root/reference
INC = -I../../oracle/_ref/include -I$(REF)
all: djpeg_client djpeg_bench
djpeg_client: djpeg_client.c
	gcc -O2 -Wall $(INC) -o $@ $< -L../../oracle/_ref -l:libjpeg.so.62 -lpthread
# measurement tool of tools/bench_djpeg_dropin.py
djpeg_bench: djpeg_bench.c
	gcc -O2 -Wall $(INC) -o $@ $< -L../../oracle/_ref -l:libjpeg.so.62 -lpthread
