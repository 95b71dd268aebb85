[BTLCountingBloomFilter_v1]
	BloomFilterSize = 1
	HashNum = 2
	KmerSize = 8
	BloomFilterSizeInBytes = 8
	BitsPerCounter = 8
[HeaderEnd]
ÿÿÿÿÿÿÿÿ